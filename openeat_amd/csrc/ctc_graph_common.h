// What the graph CTC decoders share (ctc_graph.hip, ctc_graph_beam.hip, ctc_graph_nbest.hip): the tie rule and the host checks their
// entries have in common.
#pragma once
#include "oe_common.h"

#define GRAPH_MAX_T (1 << 20)

// the tie rule (oe_ctc_align's, generalised): the greater value, the lower index among equal values
__device__ __forceinline__ bool graph_better(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

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
