#!/usr/bin/env python3
"""N-best grammar-constrained CTC decoding on the device (oe_ctc_graph_nbest) beside the dense 1-best (oe_ctc_graph) (GPU box).

  python tools/ctc_graph_nbest_bench.py [--out FILE]

The shape of tools/ctc_graph_decode_bench.py, B = 32 utterances of T = 250 frames, V = 4233, and its planted logits; two graphs:
  trie_loop    1000 phrases of 6 random labels as a prefix trie, every phrase returning to the start (a few thousand arcs;
               the start node has 1000 arcs in)
  lexicon      1000 words of 3 labels, each a chain of its own from the start node back to it: one node with 1000 arcs in
               and 1000 out, no shared prefixes
For K = 1, 2, 4, 8 and both `distinct` modes the call is timed with HIP events (median of 5 after a warm-up, three runs, the
middle one); launch 1 is oe_ctc_kws's (lp_rows_kernel, one kernel for both) and is timed alone through oe_ctc_kws, as the decode bench
does, so the recursion launch is the call minus that.  oe_ctc_graph at the same shape stands beside it: the dense kernel is
the yardstick, and `ratio` is recursion launch / dense recursion launch.  The call is also checked at the size it is timed at:
with K = 1 the score and the arcs must be oe_ctc_graph's, and on trie_loop rank 0 must spell the planted tokens.  One JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_graph_decode_bench as D  # noqa: E402
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import DecodingGraph  # noqa: E402

DEV = "cuda"
B, T, V = D.B, D.T, D.V
MODES = {"arcs": hip.CTC_GRAPH_NBEST_ARCS, "tokens": hip.CTC_GRAPH_NBEST_TOKENS}


def lexicon(seed, words=1000, length=3):
    rng = np.random.default_rng(seed)
    arcs, node = [], 1
    for _ in range(words):
        y = 1 + np.cumsum(rng.integers(1, V - 1, size=length)) % (V - 1)        # never the same label twice in a row
        at = 0
        for i, c in enumerate(y):
            nxt = 0 if i == length - 1 else node
            arcs.append((at, nxt, int(c), 0.0))
            if nxt:
                node += 1
            at = nxt
    return DecodingGraph(node, arcs, {0: 0.0})


class Run:
    def __init__(self, logits, graph, K, distinct):
        self.lib, self.graph, self.K = hip.lib(), graph, K
        self.g = hip.decoding_graph(graph, DEV)
        self.nbytes = self.lib.oe_ctc_graph_nbest_workspace_bytes(B, T, len(graph.cols), graph.num_nodes, graph.num_arcs, K)
        assert self.nbytes > 0
        self.keep = [torch.empty(self.nbytes, dtype=torch.uint8, device=DEV), torch.full((B,), T, dtype=torch.int32, device=DEV),
                     torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, K, device=DEV), torch.empty(B, K, dtype=torch.int32, device=DEV),
                     torch.empty(B, K, T, dtype=torch.int32, device=DEV), torch.empty(B, K, T, dtype=torch.int32, device=DEV), logits]
        ws, hl, n_hyp, score, length, arcs, toks, _ = self.keep
        a = self.a = hip.CtcGraphNbestArgs()
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, hl.data_ptr()
        a.graph, a.normalized, a.nbest, a.distinct, a.max_len, a.workspace = C.pointer(self.g), 0, K, MODES[distinct], T, ws.data_ptr()
        a.n_hyp, a.hyp_score, a.hyp_len, a.hyp_arcs, a.hyp_tokens = (t.data_ptr() for t in (n_hyp, score, length, arcs, toks))

    def __call__(self):
        hip.check(self.lib.oe_ctc_graph_nbest(C.byref(self.a), hip.stream()), "oe_ctc_graph_nbest")

    def best(self):
        """-> rank 0 of every utterance: its arcs, its score; and n_hyp."""
        torch.cuda.synchronize()
        n, sc, ln, ar = (t.cpu().numpy() for t in self.keep[2:6])
        return [ar[b, 0, : max(ln[b, 0], 0)].tolist() for b in range(B)], sc[:, 0], n


def part(name, logits, graph, want_tokens):
    dense = D.Run(logits, graph)
    dense()
    torch.cuda.synchronize()
    d_score = dense.keep[2].cpu().numpy()
    d_n, d_arc = dense.keep[6].cpu().numpy(), dense.keep[7].cpu().numpy()
    assert np.isfinite(d_score).all(), f"{name}: an utterance is infeasible"
    ms_dense, runs_dense = D.middle(dense)
    ms_rows, runs_rows = D.rows_alone(logits, graph.cols)
    rows = []
    for distinct in MODES:
        for K in (1, 2, 4, 8):
            run = Run(logits, graph, K, distinct)
            run()
            arcs, score, n = run.best()
            assert (n == K).all(), f"{name} K={K} {distinct}: n_hyp {n.tolist()}"
            if K == 1:
                assert score.tobytes() == d_score.tobytes(), f"{name} {distinct}: the 1-best score is not oe_ctc_graph's"
                assert all(arcs[b] == d_arc[b, : d_n[b]].tolist() for b in range(B)), f"{name} {distinct}: the 1-best arcs are not oe_ctc_graph's"
            if want_tokens is not None:
                bad = [b for b in range(B) if graph.label[arcs[b]].tolist() != want_tokens[b]]
                assert not bad, f"{name} K={K} {distinct}: utterances {bad[:5]} did not decode to the planted tokens"
            ms, runs = D.middle(run)
            rows.append({"K": K, "distinct": distinct, "call_ms": round(ms, 3), "call_runs_ms": runs, "launch2_ms": round(ms - ms_rows, 3),
                         "launch2_us_per_frame": round((ms - ms_rows) * 1e3 / T, 2),
                         "ratio_to_dense_launch2": round((ms - ms_rows) / (ms_dense - ms_rows), 2),
                         "workspace_MiB": round(run.nbytes / 2 ** 20, 1),
                         "record_table_MiB": round(4 * B * T * graph.num_arcs * K / 2 ** 20, 1)})
            del run
    return {"graph": name, "Q": graph.num_nodes, "A": graph.num_arcs, "U": len(graph.cols), "max_in_degree": int(np.diff(graph.in_ptr).max()),
            "launch1_ms": round(ms_rows, 3), "launch1_runs_ms": runs_rows,
            "dense": {"call_ms": round(ms_dense, 3), "call_runs_ms": runs_dense, "launch2_ms": round(ms_dense - ms_rows, 3),
                      "launch2_us_per_frame": round((ms_dense - ms_rows) * 1e3 / T, 2)},
            "nbest": rows}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_graph_nbest_bench needs a GPU"
    ph = D.phrases(7)
    logits, tokens = D.planted(ph, 11)
    res = {"bench": "ctc_graph_nbest", "device": torch.cuda.get_device_name(0), "B": B, "T": T, "V": V,
           "graphs": [part("trie_loop", logits, DecodingGraph.from_phrases(ph, loop=True), tokens),
                      part("lexicon", logits, lexicon(13), None)]}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
