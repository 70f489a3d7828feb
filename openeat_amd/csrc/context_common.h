// The context graph's arguments and the automaton's step, shared by the kernels that read a ContextGraph on the device
// (beam.hip: the automaton state of every prefix inside the biased prefix beam search; context.hip: the bias of candidate
// next tokens of growing hypotheses).
// Layout, hits, k and bias: include/openeat_hip.h (oe_context_graph, oe_ctc_prefix_beam) and openeat_amd/utils/context_graph.py.
#pragma once
#include <math.h>
#include "oe_common.h"
#include "../../include/openeat_hip.h"
#include "ngram_common.h"

struct CtxGraph {          // the fields of an oe_context_graph as the kernels take them
    const uint4* __restrict__ edges;
    unsigned long long edge_mask;   // capacity - 1
    const int* __restrict__ fail;
    const int2* __restrict__ out;   // (score bits, link)
    const int* __restrict__ pend;
    int edge_max_probe, n_states;
    float c;
};

// hits + (double)c * k, the product rounded before the sum
__device__ __forceinline__ double pb_bias(double hits, float c, int k) {
#pragma clang fp contract(off)
    const double credit = (double)c * (double)k;
    return hits + credit;
}

// hits grows by the scores of the phrases that end in state ns, the list ns, link[ns], .. added one by one, longest first
__device__ __forceinline__ void pb_ctx_ends(const CtxGraph& g, int ns, double& hits) {
    int t = ns;
    for (int d = 0; d < 32 && t > 0 && t < g.n_states; ++d) {
        const int2 o = g.out[t];
        hits = hits + (double)__int_as_float(o.x);
        t = o.y;
    }
}

// The automaton's step for a prefix that sits in `state` and takes token `tok`: the new state; hits grows by the scores of
// the phrases that end there, longest first.  Every index read from a table is checked against n_states.
__device__ __forceinline__ int pb_ctx_step(const CtxGraph& g, int state, int tok, double& hits) {
    int ns = 0;
    for (int d = 0; d <= 32; ++d) {                                // depth falls with every fail link: <= 32 of them, 33 probes
        float nxt, unused;
        const unsigned long long key = ((unsigned long long)(unsigned)state << 32) | (unsigned)tok;
        if (ng_find(g.edges, g.edge_mask, g.edge_max_probe, key, nxt, unused) >= 0) { ns = __float_as_int(nxt); break; }
        if (state == 0) break;
        state = g.fail[state];
        if ((unsigned)state >= (unsigned)g.n_states) break;
    }
    if ((unsigned)ns >= (unsigned)g.n_states) ns = 0;
    pb_ctx_ends(g, ns, hits);
    return ns;
}

// Host: the checks every entry point makes on an oe_context_graph's numbers (include/openeat_hip.h; fn: the entry point's
// name, for the messages; the struct's pointers are the caller's to check), then the graph as the kernels take it.
static inline int ctx_graph_args(const char* fn, const oe_context_graph* g, CtxGraph* o) {
    OE_REQUIRE(g->n_states >= 1 && g->n_states <= (1 << 20), "%s: n_states must be 1..2^20 (got %d)", fn, g->n_states);
    OE_REQUIRE(g->capacity >= 2 && (g->capacity & (g->capacity - 1)) == 0, "%s: the graph's capacity must be a power of two >= 2 (got %ld)",
               fn, g->capacity);
    OE_REQUIRE(g->max_probe >= 0 && g->max_probe < g->capacity, "%s: bad max_probe %d of the graph", fn, g->max_probe);
    OE_REQUIRE(isfinite(g->c) && g->c >= 0.f, "%s: the partial credit c must be finite and >= 0", fn);
    o->edges = (const uint4*)g->edges; o->edge_mask = (unsigned long long)(g->capacity - 1); o->edge_max_probe = g->max_probe;
    o->fail = g->fail; o->out = (const int2*)g->out; o->pend = g->pend; o->n_states = g->n_states; o->c = g->c;
    return 0;
}
