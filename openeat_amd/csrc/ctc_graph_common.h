// What the graph CTC kernels share (ctc_graph.hip, ctc_graph_beam.hip, ctc_graph_nbest.hip, ctc_graph_beam_logp.hip): the tie rule, the
// push key and the list append of the token-passing kernels, and the host checks their entries have in common.
#pragma once
#include "oe_common.h"

#define GRAPH_MAX_T (1 << 20)

// the tie rule (oe_ctc_align's, generalised): the greater value, the lower index among equal values
__device__ __forceinline__ bool graph_better(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

typedef unsigned long long beam_u64;

// (value, arc id) -> a key whose unsigned order is "greater value, then lower id"; 0 is below every key.  -0 and +0 are one value.
__device__ __forceinline__ beam_u64 beam_key(float v, int id) {
    const unsigned u = __float_as_uint(v + 0.f);
    const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((beam_u64)o << 32) | (unsigned)~id;
}
__device__ __forceinline__ int beam_key_id(beam_u64 k) { return (int)~(unsigned)k; }
__device__ __forceinline__ beam_u64 beam_load(const beam_u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void beam_clear(beam_u64* p) { __hip_atomic_store(p, (beam_u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A slot in a list for every lane that wants one, one add per wave.  Called by whole waves only (uniform control flow).
__device__ __forceinline__ int beam_append(int* counter, bool want) {
    const beam_u64 m = __ballot(want);
    if (m == 0) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader, 64);
    return want ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

// The checks the decoders' entries share; graph: oe_decoding_graph or oe_beam_graph.  max_trav: null where the entry has none.
template <class Graph>
static int graph_check(const char* name, const Graph* graph, const float* logits, long ldv, int B, int T, int V, const int* hlens,
                       const void* workspace, const int* max_trav) {
    OE_REQUIRE(graph, "%s: null graph", name);
    OE_REQUIRE(logits, "%s: null logits", name);
    OE_REQUIRE(hlens, "%s: null hlens", name);
    OE_REQUIRE(workspace, "%s: null workspace", name);
    OE_REQUIRE(B > 0 && T > 0 && T <= GRAPH_MAX_T && V > 1 && ldv >= V, "%s: bad shape B=%d T=%d V=%d ldv=%ld (1 <= B, 1 <= T <= 2^20, ldv >= V)",
               name, B, T, V, ldv);
    OE_REQUIRE(graph->U >= 1 && graph->U < V, "%s: U=%d distinct labels outside 1 .. V-1 = %d", name, graph->U, V - 1);
    OE_REQUIRE(!max_trav || *max_trav >= 1, "%s: max_trav=%d < 1", name, max_trav ? *max_trav : 0);
    OE_REQUIRE((((uintptr_t)workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", name);
    return 0;
}
