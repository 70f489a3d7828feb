// Back-off n-gram (ARPA) language-model scores of all B x beam hypotheses on the device, one wavefront per hypothesis
// (the reference's openeat/models/asr_model.py:515-516: `lm.score(' '.join(content), bos=True, eos=True)` per hypothesis on
// the host, with kenlm).  Semantics in include/openeat_hip.h; the host twin is openeat_amd/models/ngram_lm.py.
//
// Lookup structure: chained exact keys in one open-addressing table (linear probing, power-of-two capacity >= 2 x the
// number of n-grams of order >= 2, i.e. load factor <= 0.5).  Every listed n-gram has an entry number: a unigram's is its
// word id, an n-gram of order >= 2 has n_words + the slot it sits in.  Its key is (entry of its first k-1 words) << 32 |
// (id of its k-th word): the key IS the n-gram, no hash is ever compared, so a listed n-gram is found exactly and an
// unlisted one is never mistaken for a listed one.  A slot is 16 bytes {key, log10 p, back-off}: one load answers a
// probe.  The builder records the longest displacement any key has (max_probe); a lookup ends at the key, at an empty
// slot, or after max_probe + 1 slots, whichever comes first, and every slot index is masked by capacity - 1.
//
// What is parallel.  The term of position i is  logp(w[i-k+1..i])  for the longest listed k  plus the back-offs of the
// contexts w[i-j+1..i-1], j > k, that are listed.  All of these are properties of the n-grams that START at some
// position s: the chain  w[s], w[s..s+1], .. w[s..s+order-1]  (each found from the one before, so order-1 dependent
// probes, stopping at the first that is not listed - the reader guarantees that a listed n-gram's prefix is listed).  So
// a lane walks the chain of ONE start position and leaves (how many were found, their log10 p, their back-offs) in LDS;
// then a lane collects the term of ONE scored position from the order chains that cover it.  That is order-1 probes per
// position instead of the order (order+1) / 2 - 1 a per-position search makes, and the 64 chains of a tile are
// independent loads in flight together.  Tiles of 64 positions; the last order-1 chains of a tile stay in LDS for the next.
// Sums are float64: a lane adds its positions' terms in tile order, then a xor-butterfly over the wave - a fixed order,
// so a score is the same bits on every run.  No atomics.
//
// Bound: latency.  A hypothesis of L tokens is ceil((L + 2) / 64) tiles of order-1 dependent 16-byte gathers into a table
// that does not fit LDS (32 MiB for a million n-grams); the bytes moved are a few MB per call.
#include <math.h>
#include "oe_common.h"
#include "../../include/openeat_hip.h"
#include "ngram_common.h"

#define NG_TILE 64
#define NG_COLS (NG_TILE + NG_MAXORDER - 1)

__global__ __launch_bounds__(64) void ngram_score_kernel(NgModel m, const int* __restrict__ tokens, long ld,
                                                         const int* __restrict__ lens, int bos, int eos, double* __restrict__ score,
                                                         double* __restrict__ tok_logp, int* __restrict__ tok_order) {
    __shared__ int wd[NG_COLS];                                  // word ids of positions base .. base + 63 + (order-1)
    __shared__ int found[NG_COLS];                               // column c = start position base - (NG_MAXORDER-1) + c
    __shared__ float lp[NG_MAXORDER][NG_COLS], bo[NG_MAXORDER][NG_COLS];

    const int r = blockIdx.x, lane = threadIdx.x;
    const int len_raw = lens[r];
    if (len_raw < 0) {                                           // the slot does not exist (wave-uniform)
        if (lane == 0) score[r] = -__builtin_huge_val();
        return;
    }
    const int len = (int)min((long)len_raw, ld);
    const int off = bos ? 1 : 0;
    const int P = off + len + (eos ? 1 : 0);                     // positions: [<s>] tokens [</s>]; scored: off .. P-1
    const int* tk = tokens + (long)r * ld;
    const int H = NG_MAXORDER - 1;

    if (lane < H) found[lane] = 0;                               // no chain starts before position 0
    double acc = 0.0;
    for (int base = 0; base < P; base += NG_TILE) {
        // ---- word ids of the tile and of the order-1 positions after it
        for (int c = lane; c < NG_COLS; c += NG_TILE) {
            const int q = base + c;
            int w = -1;
            if (q < P) {
                if (q < off) w = m.bos_word;
                else if (q - off < len) w = ng_word(m, tk[q - off]);
                else w = m.eos_word;
            }
            wd[c] = w;
        }
        __syncthreads();
        // ---- the chain that starts at position s = base + lane
        {
            const int s = base + lane;
            int nf = 0;
            if (s < P) {
                long e = wd[lane];
                const float2 u = m.unigrams[e];
                lp[0][H + lane] = u.x; bo[0][H + lane] = u.y;
                nf = 1;
                for (int k = 2; k <= m.order; ++k) {
                    if (s + k - 1 >= P) break;
                    const unsigned long long key = ((unsigned long long)e << 32) | (unsigned)wd[lane + k - 1];
                    float a = 0.f, b = 0.f;
                    const long slot = ng_find(m.table, m.mask, m.max_probe, key, a, b);
                    if (slot < 0) break;
                    lp[k - 1][H + lane] = a; bo[k - 1][H + lane] = b;
                    e = (long)m.n_words + slot;
                    nf = k;
                }
            }
            found[H + lane] = nf;
        }
        __syncthreads();
        // ---- the term of position i = base + lane: longest listed n-gram ending at i, back-offs of the longer contexts
        {
            const int i = base + lane;
            if (i >= off && i < P) {
                double term = 0.0;
                int k = min(m.order, i + 1);
                for (; k > 1; --k) {
                    const int c = H + lane - (k - 1);            // chain that starts at i - k + 1
                    const int nf = found[c];
                    if (nf >= k) break;
                    if (nf >= k - 1) term += (double)bo[k - 2][c];        // its context w[i-k+1 .. i-1] is listed
                }
                term += (double)lp[k - 1][H + lane - (k - 1)];
                acc += term;
                const long o = (long)r * (ld + 1) + (i - off);
                if (tok_logp) tok_logp[o] = term;
                if (tok_order) tok_order[o] = k;
            }
        }
        __syncthreads();
        // ---- keep the last order-1 chains for the next tile
        float keep_lp[NG_MAXORDER], keep_bo[NG_MAXORDER];
        int keep_f = 0;
        if (lane < H) {
            keep_f = found[NG_TILE + lane];
#pragma unroll
            for (int k = 0; k < NG_MAXORDER; ++k) { keep_lp[k] = lp[k][NG_TILE + lane]; keep_bo[k] = bo[k][NG_TILE + lane]; }
        }
        __syncthreads();
        if (lane < H) {
            found[lane] = keep_f;
#pragma unroll
            for (int k = 0; k < NG_MAXORDER; ++k) { lp[k][lane] = keep_lp[k]; bo[k][lane] = keep_bo[k]; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += oe_shfl_xor_f64(acc, o);
    if (lane == 0) score[r] = acc;
}

extern "C" int oe_ngram_score(const oe_ngram_model* model, const int* tokens, long ld, const int* lens, int R, int bos, int eos,
                              double* score, double* tok_logp, int* tok_order, void* stream) {
    OE_REQUIRE(model && model->unigrams && model->table && model->tok2word && tokens && lens && score, "oe_ngram_score: null pointer");
    NgModel m;
    if (ng_model_args("oe_ngram_score", model, &m)) return -1;
    OE_REQUIRE(R >= 0 && m.V > 0 && ld >= 0, "oe_ngram_score: bad shape R=%d V=%d ld=%ld", R, m.V, ld);
    if (R == 0) return 0;
    hipLaunchKernelGGL(ngram_score_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, m, tokens, ld, lens, bos, eos, score, tok_logp,
                       tok_order);
    OE_LAUNCH_CHECK("ngram_score");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The LM term of every candidate next token of every hypothesis (oe_ngram_next; semantics in include/openeat_hip.h): what a
// search step needs, where ngram_score_kernel scores finished sequences.  One block = one wave = one hypothesis x one slice
// of NGN_SLICE candidates; grid (R, slices).
//
// The context is the last n = min(order-1, len+1) words of <s> + hypothesis.  Its suffixes of 1..n words are the only
// dependent probes: lane j-1 walks the suffix of j words (j-1 probes, each entry found from the one before) and leaves
// (is it listed, its entry number, its back-off) in LDS - once per block, at most order-2 probes deep.  Then every lane
// owns NGN_PER candidates: from the longest listed suffix down, one lookup of (suffix's entry, word) per level until the
// n-gram is listed, the back-off of the level added where it is not; then the unigram.  A suffix that is not listed adds
// nothing and is not probed (its extensions cannot be listed).  The first slot of a level is read for all of a lane's
// candidates before any is compared, and the unigrams before the levels: the loads of a lane do not wait for one another.
// A term is a float64 sum in the order of ngram_score_kernel (back-offs longest first, then the log10 p) of the same float32
// values, so it is the same bits, for any candidate order and any grid shape.
//
// Bound: latency / gather.  R x C x (listed levels) independent 16-byte reads into a table far larger than LDS.
#define NGN_PER 4
#define NGN_SLICE (OE_WAVE * NGN_PER)

__global__ __launch_bounds__(OE_WAVE) void ngram_next_kernel(NgModel m, const int* __restrict__ tokens, long ld,
                                                             const int* __restrict__ lens, const int* __restrict__ cand, int C,
                                                             int eos_tok, double* __restrict__ out) {
    __shared__ int wd[NG_MAXORDER];                              // the context's words, oldest first
    __shared__ int listed[NG_MAXORDER];                          // [j]: the suffix of j words, j = 1 .. n
    __shared__ unsigned ent[NG_MAXORDER];
    __shared__ float bo[NG_MAXORDER];

    const int r = blockIdx.x, lane = threadIdx.x;
    const long j0 = (long)blockIdx.y * NGN_SLICE + lane;         // this lane's candidates: j0 + u * 64
    double* o = out + (long)r * C;
    const int len_raw = lens[r];
    if (len_raw < 0) {                                           // the slot does not exist (wave-uniform)
#pragma unroll
        for (int u = 0; u < NGN_PER; ++u)
            if (j0 + u * OE_WAVE < C) o[j0 + u * OE_WAVE] = -__builtin_huge_val();
        return;
    }
    const int len = (int)min((long)len_raw, ld);
    const int P = len + 1;                                       // <s> and the tokens
    const int n = min(m.order - 1, P);
    if (lane < n) {
        const int q = P - n + lane;
        wd[lane] = q == 0 ? m.bos_word : ng_word(m, tokens[(long)r * ld + (q - 1)]);
    }
    __syncthreads();
    if (lane < n) {                                              // the suffix of j = lane + 1 words: wd[n-j .. n-1]
        const int j = lane + 1;
        long e = wd[n - j];
        float a = 0.f, b = m.unigrams[e].y;
        int ok = 1;
        for (int k = 1; k < j; ++k) {
            const unsigned long long key = ((unsigned long long)e << 32) | (unsigned)wd[n - j + k];
            const long slot = ng_find(m.table, m.mask, m.max_probe, key, a, b);
            if (slot < 0) { ok = 0; break; }
            e = (long)m.n_words + slot;
        }
        listed[j] = ok; ent[j] = (unsigned)e; bo[j] = b;
    }
    __syncthreads();

    unsigned w[NGN_PER];
    float uni[NGN_PER];
    double term[NGN_PER];
    bool open[NGN_PER];                                          // a candidate whose n-gram is not found yet
#pragma unroll
    for (int u = 0; u < NGN_PER; ++u) {
        const long j = j0 + u * OE_WAVE;
        open[u] = j < C;
        term[u] = 0.0;
        w[u] = 0; uni[u] = 0.f;
        if (open[u]) {
            const int tok = cand ? cand[(long)r * C + j] : (int)j;
            w[u] = (unsigned)((eos_tok >= 0 && tok == eos_tok) ? m.eos_word : ng_word(m, tok));
            uni[u] = m.unigrams[w[u]].x;
        }
    }
    for (int j = n; j >= 1; --j) {
        if (!listed[j]) continue;                                // wave-uniform
        const unsigned long long hi = (unsigned long long)ent[j] << 32;
        const double b = (double)bo[j];
        unsigned long long slot[NGN_PER];
        uint4 v[NGN_PER];
#pragma unroll
        for (int u = 0; u < NGN_PER; ++u) {
            slot[u] = ng_mix(hi | w[u]) & m.mask;
            if (open[u]) v[u] = m.table[slot[u]];
        }
#pragma unroll
        for (int u = 0; u < NGN_PER; ++u) {
            if (!open[u]) continue;
            const unsigned long long key = hi | w[u];
            for (int d = 0;; ++d) {                              // ng_find's walk: the key, an empty slot, or max_probe + 1 slots
                const unsigned long long k = ((unsigned long long)v[u].y << 32) | v[u].x;
                if (k == key) { term[u] += (double)__uint_as_float(v[u].z); open[u] = false; break; }
                if (k == NG_EMPTY || d == m.max_probe) { term[u] += b; break; }
                slot[u] = (slot[u] + 1) & m.mask;
                v[u] = m.table[slot[u]];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NGN_PER; ++u) {
        const long j = j0 + u * OE_WAVE;
        if (j < C) o[j] = open[u] ? term[u] + (double)uni[u] : term[u];
    }
}

extern "C" int oe_ngram_next(const oe_ngram_model* model, const int* tokens, long ld, const int* lens, int R, const int* cand, int C,
                             int eos_tok, double* out, void* stream) {
    OE_REQUIRE(model && model->unigrams && model->table && model->tok2word && tokens && lens && out, "oe_ngram_next: null pointer");
    NgModel m;
    if (ng_model_args("oe_ngram_next", model, &m)) return -1;
    OE_REQUIRE(R >= 0 && m.V > 0 && ld >= 0, "oe_ngram_next: bad shape R=%d V=%d ld=%ld", R, m.V, ld);
    OE_REQUIRE(C >= 1, "oe_ngram_next: C must be >= 1 (got %d)", C);
    OE_REQUIRE(cand || C == m.V, "oe_ngram_next: without cand every token is scored: C must equal V = %d (got %d)", m.V, C);
    OE_REQUIRE(eos_tok >= -1 && eos_tok < m.V, "oe_ngram_next: eos_tok %d outside -1..%d", eos_tok, m.V - 1);
    if (R == 0) return 0;
    const int slices = (int)(((long)C + NGN_SLICE - 1) / NGN_SLICE);
    OE_REQUIRE(slices <= 65535, "oe_ngram_next: C = %d needs more than 65535 slices of %d candidates", C, NGN_SLICE);
    hipLaunchKernelGGL(ngram_next_kernel, dim3(R, slices), dim3(OE_WAVE), 0, (hipStream_t)stream, m, tokens, ld, lens, cand, C, eos_tok,
                       out);
    OE_LAUNCH_CHECK("ngram_next");
    return 0;
}
