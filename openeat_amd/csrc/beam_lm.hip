// CTC prefix beam search with n-gram LM shallow fusion on the device, one wavefront per utterance: the recursion of
// beam.hip (read its header first: what an entry of next_hyps can receive in one frame, the first-touch stamp, prefixes as
// (hash, length), back-pointers) with ONE change - the key that orders next_hyps before the cut to `beam` is
//   total(p) = log_add(pb, pnb) + lm_weight * LM(p) + length_bonus * len(p)
// (semantics in include/openeat_hip.h, oe_ctc_prefix_beam_lm).  The pb / pnb arithmetic is beam.hip's, statement for
// statement (pbl_log_add* are its pb_log_add*), so out_ctc is the same bits as oe_ctc_prefix_beam's score wherever both
// searches keep the same prefixes.
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
// What is parallel, on top of beam.hip: the probes of all beam x beam extension candidates that are NEW prefixes (lane =
// pair, as there).  A "stay" entry and an extension that lands on a prefix already in the beam keep that prefix's lm and
// state and probe nothing.  Candidates carry only the lm VALUE in registers; after the selection the <= beam winners that
// are new prefixes redo their probes (one lane each) to write the state of the next frame.
// Bound: latency.  A frame adds two rounds of <= order-1 independent 16-byte gathers into a table that does not fit LDS.
#include <math.h>
#include "oe_common.h"
#include "../../include/openeat_hip.h"
#include "ngram_common.h"

#define PBL_MAXBEAM 16
#define PBL_MAXC ((PBL_MAXBEAM * PBL_MAXBEAM + 63) / 64)       // (token, hypothesis) pairs per lane
#define PBL_HASH_MUL 0x9E3779B97F4A7C15ull
#define PBL_H (NG_MAXORDER - 1)                                // contexts kept per prefix

__device__ __forceinline__ double pbl_neg() { return -__builtin_huge_val(); }
// beam.hip's pb_term / pb_log_add2 / pb_log_add3, unchanged (the reasons for their shape are written there)
__device__ __forceinline__ double pbl_term(double x, double m) {
    return x == m ? 1.0 : (x == pbl_neg() ? 0.0 : exp(x - m));
}
__device__ __forceinline__ double pbl_log_add2(double a, double b) {
    const double ninf = pbl_neg();
    if (a == ninf && b == ninf) return ninf;
    const double m = fmax(a, b);
    return m + log(pbl_term(a, m) + pbl_term(b, m));
}
__device__ __forceinline__ double pbl_log_add3(double a, double b, double c) {
    const double ninf = pbl_neg();
    if (a == ninf && b == ninf && c == ninf) return ninf;
    const double m = fmax(a, fmax(b, c));
    return m + log(pbl_term(a, m) + pbl_term(b, m) + pbl_term(c, m));
}
__device__ __forceinline__ double pbl_shfl_xor(double v, int o) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, o, 64);
    hi = __shfl_xor(hi, o, 64);
    return __hiloint2double(hi, lo);
}
// (ctc + lm_weight * lm) + length_bonus * len with every product and sum rounded on its own, as a host float64 expression
// is: a fused multiply-add would move a total by an ulp and with it the order of two entries that tie exactly.
__device__ __forceinline__ double pbl_total(double ctc, double lm, int len, double lm_weight, double length_bonus) {
#pragma clang fp contract(off)
    const double a = lm_weight * lm;
    const double c = length_bonus * (double)len;
    return (ctc + a) + c;
}

struct PblModel {       // the arguments of oe_ngram_score that describe the model
    const float2* unigrams;
    const uint4* table;
    const int* tok2word;
    unsigned long long mask;
    int n_words, max_probe, order, bos_word, eos_word, unk_word, V;
};

__device__ __forceinline__ int pbl_word(const PblModel& m, int tok) {
    int w = (tok >= 0 && tok < m.V) ? m.tok2word[tok] : m.unk_word;
    if (w < 0 || w >= m.n_words) w = m.unk_word;
    return w;
}

// log10 p(w | the prefix whose state is ent / bo); ent_out / bo_out (or null): the state of prefix + w
__device__ __forceinline__ double pbl_extend(const PblModel& m, const int* ent, const float* bo, int w, int* ent_out, float* bo_out) {
    const int H = m.order - 1;
    const float2 u = m.unigrams[w];
    int ce[PBL_H], he[PBL_H];
    float cb[PBL_H], hl[PBL_H], hb[PBL_H];
#pragma unroll
    for (int j = 0; j < PBL_H; ++j) {
        ce[j] = j < H ? ent[j] : -1;
        cb[j] = j < H ? bo[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < PBL_H; ++j) {                              // the (j+2)-gram: context of j+1 words, then w
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
    for (int j = 0; j < PBL_H; ++j)
        if (he[j] >= 0) { K = j + 2; lp = hl[j]; }
    double term = (double)lp;
#pragma unroll
    for (int j = 0; j < PBL_H; ++j)
        if (j + 1 >= K && ce[j] >= 0) term = (double)cb[j] + term;
    if (ent_out) {
        ent_out[0] = w; bo_out[0] = u.y;
#pragma unroll
        for (int j = 1; j < PBL_H; ++j) { ent_out[j] = he[j - 1]; bo_out[j] = hb[j - 1]; }
    }
    return term;
}

struct PblHyp {         // one entry of next_hyps
    unsigned long long key;
    double pb, pnb, lm, total;
    int len, last, parent, tok, order;
};

__global__ __launch_bounds__(64) void ctc_prefix_beam_lm_kernel(const float* __restrict__ topk_logp, const long long* __restrict__ topk_idx,
                                                                int Tmax, const int* __restrict__ lens, int beam, int max_len,
                                                                PblModel m, double lm_weight, double length_bonus, int eos,
                                                                int* __restrict__ hist, int* __restrict__ out_prefix,
                                                                int* __restrict__ out_len, double* __restrict__ out_score,
                                                                double* __restrict__ out_ctc, double* __restrict__ out_lm,
                                                                int* __restrict__ status) {
    __shared__ unsigned long long cur_key[PBL_MAXBEAM];
    __shared__ double cur_pb[PBL_MAXBEAM], cur_pnb[PBL_MAXBEAM], cur_lm[PBL_MAXBEAM];
    __shared__ int cur_len[PBL_MAXBEAM], cur_last[PBL_MAXBEAM];
    __shared__ int cur_ent[PBL_MAXBEAM][PBL_H];
    __shared__ float cur_bo[PBL_MAXBEAM][PBL_H];
    __shared__ double tk_ps[PBL_MAXBEAM];
    __shared__ int tk_s[PBL_MAXBEAM], tk_w[PBL_MAXBEAM];
    __shared__ int con_has[PBL_MAXBEAM], con_from[PBL_MAXBEAM], con_three[PBL_MAXBEAM], con_order[PBL_MAXBEAM];
    __shared__ double con_a[PBL_MAXBEAM], con_b[PBL_MAXBEAM];
    __shared__ unsigned long long nx_key[PBL_MAXBEAM];
    __shared__ double nx_pb[PBL_MAXBEAM], nx_pnb[PBL_MAXBEAM], nx_lm[PBL_MAXBEAM];
    __shared__ int nx_len[PBL_MAXBEAM], nx_last[PBL_MAXBEAM], nx_parent[PBL_MAXBEAM], nx_tok[PBL_MAXBEAM];
    __shared__ int nx_ent[PBL_MAXBEAM][PBL_H];
    __shared__ float nx_bo[PBL_MAXBEAM][PBL_H];
    __shared__ double fin_total[PBL_MAXBEAM];

    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = min(lens ? lens[b] : Tmax, Tmax);
    const double NEG = pbl_neg();
    int ncur = 1;
    if (lane == 0) {
        cur_key[0] = 0; cur_pb[0] = 0.0; cur_pnb[0] = NEG; cur_len[0] = 0; cur_last[0] = -1; cur_lm[0] = 0.0;
        cur_ent[0][0] = m.bos_word; cur_bo[0][0] = m.unigrams[m.bos_word].y;          // the context <s>
#pragma unroll
        for (int j = 1; j < PBL_H; ++j) { cur_ent[0][j] = -1; cur_bo[0][j] = 0.f; }
    }
    __syncthreads();
    int* hist_b = hist + (long)b * Tmax * beam * 2;

    for (int t = 0; t < T; ++t) {
        if (lane < beam) {
            const long o = ((long)b * Tmax + t) * beam + lane;
            const int s = (int)topk_idx[o];
            tk_ps[lane] = (double)topk_logp[o];
            tk_s[lane] = s;
            tk_w[lane] = pbl_word(m, s);
        }
        if (lane < ncur) con_has[lane] = 0;
        __syncthreads();

        // ---- extension candidates: pair p = (j, h), lanes p, p + 64, ...
        PblHyp cand[PBL_MAXC + 1];
        bool alive[PBL_MAXC + 1];
        const int npairs = beam * ncur;
#pragma unroll
        for (int c = 0; c < PBL_MAXC; ++c) {
            const int p = lane + 64 * c;
            alive[c] = false;
            if (p < npairs) {
                const int j = p / ncur, h = p - j * ncur;
                const int s = tk_s[j];
                if (s != 0) {
                    const double ps = tk_ps[j];
                    const unsigned long long key = cur_key[h] * PBL_HASH_MUL + (unsigned long long)(s + 1);
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
                        cand[c].pnb = rep ? a : pbl_log_add3(NEG, a, bb);
                        cand[c].order = 2 * p + 1;
                        cand[c].lm = cur_lm[h] + pbl_extend(m, cur_ent[h], cur_bo[h], tk_w[j], nullptr, nullptr);
                    }
                }
            }
        }
        __syncthreads();

        // ---- the current prefixes' own entries: lane n
        alive[PBL_MAXC] = false;
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
                npb = pbl_log_add3(NEG, pb + tk_ps[j0], pnb + tk_ps[j0]);
                order = min(order, 2 * (j0 * ncur + n));
                touched = true;
            }
            const bool rep = jr >= 0, con = con_has[n] != 0;
            const bool con_first = con && (!rep || con_from[n] < n);
            if (con && con_first) npnb = con_three[n] ? pbl_log_add3(npnb, con_a[n], con_b[n]) : pbl_log_add2(npnb, con_a[n]);
            if (rep) { npnb = pbl_log_add2(npnb, pnb + tk_ps[jr]); order = min(order, 2 * (jr * ncur + n)); touched = true; }
            if (con && !con_first) npnb = con_three[n] ? pbl_log_add3(npnb, con_a[n], con_b[n]) : pbl_log_add2(npnb, con_a[n]);
            if (con) { order = min(order, con_order[n]); touched = true; }
            if (touched) {
                alive[PBL_MAXC] = true;
                PblHyp& e = cand[PBL_MAXC];
                e.key = cur_key[n]; e.len = cur_len[n]; e.last = last; e.parent = n; e.tok = -1; e.pb = npb; e.pnb = npnb; e.order = order;
                e.lm = cur_lm[n];
            }
        }
#pragma unroll
        for (int c = 0; c <= PBL_MAXC; ++c)
            if (alive[c]) cand[c].total = pbl_total(pbl_log_add2(cand[c].pb, cand[c].pnb), cand[c].lm, cand[c].len, lm_weight, length_bonus);

        // ---- the best `beam` entries by (total descending, first touch ascending)
        int nsel = 0;
        for (int r = 0; r < beam; ++r) {
            double bs = NEG;
            int bo = 0x7fffffff, bc = -1;
#pragma unroll
            for (int c = 0; c <= PBL_MAXC; ++c)
                if (alive[c] && (bc < 0 || cand[c].total > bs || (cand[c].total == bs && cand[c].order < bo))) { bs = cand[c].total; bo = cand[c].order; bc = c; }
            double ws = bs;
            int wo = bo;                                      // lanes without a candidate carry (NEG, INT_MAX)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double os = pbl_shfl_xor(ws, o);
                const int oo = __shfl_xor(wo, o, 64);
                if (oo != 0x7fffffff && (wo == 0x7fffffff || os > ws || (os == ws && oo < wo))) { ws = os; wo = oo; }
            }
            if (wo == 0x7fffffff) break;                      // nothing left (wave-uniform)
            if (bc >= 0 && bo == wo) {                        // stamps are unique: this lane holds the winner
#pragma unroll
                for (int c = 0; c <= PBL_MAXC; ++c)
                    if (c == bc) {
                        nx_key[r] = cand[c].key; nx_pb[r] = cand[c].pb; nx_pnb[r] = cand[c].pnb; nx_len[r] = cand[c].len; nx_last[r] = cand[c].last;
                        nx_lm[r] = cand[c].lm; nx_parent[r] = cand[c].parent; nx_tok[r] = cand[c].tok;
                        hist_b[((long)t * beam + r) * 2] = cand[c].parent;
                        hist_b[((long)t * beam + r) * 2 + 1] = cand[c].tok;
                        alive[c] = false;
                    }
            }
            nsel = r + 1;
        }
        __syncthreads();
        // ---- the winners' LM state: a new prefix redoes its probes, any other entry keeps its prefix's state
        if (lane < nsel) {
            const int par = nx_parent[lane], tok = nx_tok[lane];
            if (tok >= 0) {
                pbl_extend(m, cur_ent[par], cur_bo[par], pbl_word(m, tok), nx_ent[lane], nx_bo[lane]);
            } else {
#pragma unroll
                for (int j = 0; j < PBL_H; ++j) { nx_ent[lane][j] = cur_ent[par][j]; nx_bo[lane][j] = cur_bo[par][j]; }
            }
        }
        __syncthreads();
        if (lane < nsel) {
            cur_key[lane] = nx_key[lane]; cur_pb[lane] = nx_pb[lane]; cur_pnb[lane] = nx_pnb[lane]; cur_len[lane] = nx_len[lane];
            cur_last[lane] = nx_last[lane]; cur_lm[lane] = nx_lm[lane];
#pragma unroll
            for (int j = 0; j < PBL_H; ++j) { cur_ent[lane][j] = nx_ent[lane][j]; cur_bo[lane][j] = nx_bo[lane][j]; }
        }
        ncur = nsel;
        __syncthreads();
    }

    // ---- end of the utterance: the </s> term, then the survivors stably re-sorted by total
    double lm = 0.0, ctc = NEG, total = NEG;
    if (lane < ncur) {
        lm = cur_lm[lane];
        if (eos) lm = lm + pbl_extend(m, cur_ent[lane], cur_bo[lane], m.eos_word, nullptr, nullptr);
        ctc = pbl_log_add2(cur_pb[lane], cur_pnb[lane]);
        total = pbl_total(ctc, lm, cur_len[lane], lm_weight, length_bonus);
        fin_total[lane] = total;
    }
    __syncthreads();

    // ---- results: scores, lengths, tokens by walking the back-pointers
    if (lane < beam) {
        if (lane < ncur) {
            int rank = 0;
            for (int i = 0; i < ncur; ++i) {
                const double ti = fin_total[i];
                if (ti > total || (ti == total && i < lane)) ++rank;
            }
            const long o = (long)b * beam + rank;
            const int len = cur_len[lane];
            out_score[o] = total;
            out_ctc[o] = ctc;
            out_lm[o] = lm;
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
            out_ctc[o] = NEG;
            out_lm[o] = NEG;
            out_len[o] = -1;
        }
    }
}

extern "C" size_t oe_ctc_prefix_beam_lm_workspace_bytes(int B, int Tmax, int beam) {
    return ((size_t)B * (size_t)max(Tmax, 1) * (size_t)beam * 2 + 1) * sizeof(int);
}

extern "C" int oe_ctc_prefix_beam_lm(const float* topk_logp, const long long* topk_idx, int B, int Tmax, const int* lens, int beam,
                                     int max_len, const float* unigrams, int n_words, const void* table, long capacity, int max_probe,
                                     int order, int bos_word, int eos_word, int unk_word, const int* tok2word, int V,
                                     double lm_weight, double length_bonus, int eos, void* workspace, int* out_prefix, int* out_len,
                                     double* out_score, double* out_ctc, double* out_lm, void* stream) {
    OE_REQUIRE(topk_logp && topk_idx && workspace && out_prefix && out_len && out_score && out_ctc && out_lm,
               "oe_ctc_prefix_beam_lm: null pointer");
    OE_REQUIRE(unigrams && table && tok2word, "oe_ctc_prefix_beam_lm: null pointer (model)");
    OE_REQUIRE(B > 0 && Tmax >= 0 && max_len >= 0, "oe_ctc_prefix_beam_lm: bad shape B=%d Tmax=%d max_len=%d", B, Tmax, max_len);
    OE_REQUIRE(beam >= 1 && beam <= PBL_MAXBEAM, "oe_ctc_prefix_beam_lm: beam must be 1..%d (got %d)", PBL_MAXBEAM, beam);
    OE_REQUIRE(order >= 1 && order <= NG_MAXORDER, "oe_ctc_prefix_beam_lm: order must be 1..%d (got %d)", NG_MAXORDER, order);
    OE_REQUIRE(capacity >= 2 && (capacity & (capacity - 1)) == 0, "oe_ctc_prefix_beam_lm: capacity must be a power of two >= 2 (got %ld)", capacity);
    OE_REQUIRE(max_probe >= 0 && max_probe < capacity, "oe_ctc_prefix_beam_lm: bad max_probe %d", max_probe);
    OE_REQUIRE(n_words > 0 && (long)n_words + capacity < 0x7fffffffL, "oe_ctc_prefix_beam_lm: n_words + capacity must stay below 2^31");
    OE_REQUIRE(bos_word >= 0 && bos_word < n_words && eos_word >= 0 && eos_word < n_words && unk_word >= 0 && unk_word < n_words,
               "oe_ctc_prefix_beam_lm: <s> / </s> / <unk> ids outside the vocabulary");
    OE_REQUIRE(V > 0, "oe_ctc_prefix_beam_lm: bad vocabulary size V=%d", V);
    OE_REQUIRE(isfinite(lm_weight) && isfinite(length_bonus), "oe_ctc_prefix_beam_lm: lm_weight and length_bonus must be finite");
    PblModel m;
    m.unigrams = (const float2*)unigrams; m.table = (const uint4*)table; m.tok2word = tok2word;
    m.mask = (unsigned long long)(capacity - 1);
    m.n_words = n_words; m.max_probe = max_probe; m.order = order;
    m.bos_word = bos_word; m.eos_word = eos_word; m.unk_word = unk_word; m.V = V;
    int* hist = (int*)workspace;
    int* status = hist + (size_t)B * (size_t)max(Tmax, 1) * (size_t)beam * 2;     // the caller zeroes this word and reads it back
    hipLaunchKernelGGL(ctc_prefix_beam_lm_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, topk_logp, topk_idx, Tmax, lens, beam,
                       max_len, m, lm_weight, length_bonus, eos, hist, out_prefix, out_len, out_score, out_ctc, out_lm, status);
    OE_LAUNCH_CHECK("ctc_prefix_beam_lm");
    return 0;
}
