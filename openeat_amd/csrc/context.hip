// The hotword bias of every candidate next token of every hypothesis (oe_context_next; semantics in include/openeat_hip.h):
// what a search step that grows hypotheses token by token adds to its pruning key, the counterpart of oe_ngram_next for a
// context graph.  The prefix beam search (beam.hip) makes the same automaton step inside its frame loop; the step itself,
// pb_ctx_step, is in context_common.h.  The host twin is openeat_amd/utils/context_graph.py (ContextGraph.step / .bias).
//
// One block = one wave = one hypothesis x one slice of CTN_SLICE candidates; grid (R, slices).  The row's state and hits are
// read once (wave-uniform).  Every lane owns CTN_PER candidates: the first slot of the edge (state, token) is read for all of
// them before any is compared, so a lane's loads do not wait for one another.  A hypothesis that sits in the root and a
// candidate without a root edge end there, after that one probe - the common case of the full-vocabulary form.  Otherwise
// the lane finishes the probe sequence, follows fail[] (pb_ctx_step: <= 32 links), then adds the phrases that end in the new
// state, a list of <= 32 (score, link) reads that is empty for most states, and reads pend[] of the new state.
// hits' is a float64 sum in the order of pb_ctx_step of the same float32 values, the credit c * pend is rounded before it
// is added: the bits of the biased prefix search and of ContextGraph.bias, for any candidate order and any grid shape.
//
// Bound: latency / gather.  R x C independent 16-byte reads into the edge table (tens of KiB for a thousand phrases: it
// sits in L2), 8 to 20 bytes written per candidate.
#include <math.h>
#include "oe_common.h"
#include "../../include/openeat_hip.h"
#include "context_common.h"

#define CTN_PER 4
#define CTN_SLICE (OE_WAVE * CTN_PER)

__global__ __launch_bounds__(OE_WAVE) void context_next_kernel(CtxGraph g, const int* __restrict__ state, const double* __restrict__ hits,
                                                               const int* __restrict__ cand, int C, int eos_tok,
                                                               int* __restrict__ out_state, double* __restrict__ out_hits,
                                                               double* __restrict__ out_bias) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const long j0 = (long)blockIdx.y * CTN_SLICE + lane;         // this lane's candidates: j0 + u * 64
    const long row = (long)r * C;
    const int s0 = state[r];
    if ((unsigned)s0 >= (unsigned)g.n_states) {                  // the slot does not exist (wave-uniform)
#pragma unroll
        for (int u = 0; u < CTN_PER; ++u) {
            const long j = j0 + u * OE_WAVE;
            if (j >= C) continue;
            if (out_state) { out_state[row + j] = -1; out_hits[row + j] = -__builtin_huge_val(); }
            out_bias[row + j] = -__builtin_huge_val();
        }
        return;
    }
    const double h0 = hits[r];
    const unsigned long long hi = (unsigned long long)(unsigned)s0 << 32;

    int tok[CTN_PER];
    bool walk[CTN_PER];                                          // a candidate that makes a transition
    unsigned long long slot[CTN_PER];
    uint4 v[CTN_PER];
#pragma unroll
    for (int u = 0; u < CTN_PER; ++u) {
        const long j = j0 + u * OE_WAVE;
        tok[u] = 0; slot[u] = 0;
        walk[u] = false;
        if (j < C) {
            tok[u] = cand ? cand[row + j] : (int)j;
            walk[u] = !(eos_tok >= 0 && tok[u] == eos_tok);
        }
        if (walk[u]) {
            slot[u] = ng_mix(hi | (unsigned)tok[u]) & g.edge_mask;
            v[u] = g.edges[slot[u]];
        }
    }
#pragma unroll
    for (int u = 0; u < CTN_PER; ++u) {
        const long j = j0 + u * OE_WAVE;
        if (j >= C) continue;
        int ns = s0;
        double h = h0, b = h0;                                   // the eos_tok candidate: not walked, the pending credit dropped
        if (walk[u]) {
            const unsigned long long key = hi | (unsigned)tok[u];
            bool found = false;
            for (int d = 0;; ++d) {                              // ng_find's walk: the key, an empty slot, or max_probe + 1 slots
                const unsigned long long k = ((unsigned long long)v[u].y << 32) | v[u].x;
                if (k == key) { found = true; break; }
                if (k == NG_EMPTY || d == g.edge_max_probe) break;
                slot[u] = (slot[u] + 1) & g.edge_mask;
                v[u] = g.edges[slot[u]];
            }
            ns = 0;
            if (found) {
                if (v[u].z < (unsigned)g.n_states) ns = (int)v[u].z;
                pb_ctx_ends(g, ns, h);
            } else if (s0 != 0) {                                // the edge is missing: fail[] and again, from there pb_ctx_step's walk
                const int f = g.fail[s0];
                if ((unsigned)f < (unsigned)g.n_states) ns = pb_ctx_step(g, f, tok[u], h);
            }
            b = pb_bias(h, g.c, g.pend[ns]);
        }
        if (out_state) { out_state[row + j] = ns; out_hits[row + j] = h; }
        out_bias[row + j] = b;
    }
}

extern "C" int oe_context_next(const oe_context_graph* ctx, const int* state, const double* hits, int R, const int* cand, int C,
                               int eos_tok, int* out_state, double* out_hits, double* out_bias, void* stream) {
    const char* fn = "oe_context_next";
    OE_REQUIRE(ctx && state && hits && out_bias, "%s: null pointer", fn);
    OE_REQUIRE(ctx->edges && ctx->fail && ctx->out && ctx->pend, "%s: null pointer (context graph)", fn);
    OE_REQUIRE((out_state == nullptr) == (out_hits == nullptr), "%s: out_state and out_hits are given or left out together", fn);
    OE_REQUIRE(R >= 0, "%s: bad shape R=%d", fn, R);
    OE_REQUIRE(C >= 1, "%s: C must be >= 1 (got %d)", fn, C);
    OE_REQUIRE(eos_tok >= -1, "%s: eos_tok %d below -1", fn, eos_tok);
    CtxGraph g;
    if (ctx_graph_args(fn, ctx, &g)) return -1;
    if (R == 0) return 0;
    const int slices = (int)(((long)C + CTN_SLICE - 1) / CTN_SLICE);
    OE_REQUIRE(slices <= 65535, "%s: C = %d needs more than 65535 slices of %d candidates", fn, C, CTN_SLICE);
    hipLaunchKernelGGL(context_next_kernel, dim3(R, slices), dim3(OE_WAVE), 0, (hipStream_t)stream, g, state, hits, cand, C, eos_tok,
                       out_state, out_hits, out_bias);
    OE_LAUNCH_CHECK("context_next");
    return 0;
}
