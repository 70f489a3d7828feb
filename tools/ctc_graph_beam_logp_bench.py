#!/usr/bin/env python3
"""The beam-pruned graph CTC likelihood and its gradient (oe_ctc_graph_beam_logp / oe_ctc_graph_beam_logp_grad) beside their two
neighbours (GPU box).  Synthetic data, no downloads.

  python tools/ctc_graph_beam_logp_bench.py [--out FILE]

(a) lexicon: tools/ctc_graph_beam_bench.py's loop of 100 000 words, B = 8 x T = 120, V = 2000, peaked posteriors, beams 12 and 8
    with max_active = 2^17: oe_ctc_graph_beam (the max over the same graph, T and beam) against the score and the gradient call.
    logp >= the best path's score is asserted.
(b) at_the_dense_limits: tools/ctc_graph_logp_bench.py's looped trie of 800 phrases (3927 nodes, 4726 arcs), B = 32 x T = 250,
    V = 4233: oe_ctc_graph_logp / oe_ctc_graph_logp_grad (the state in LDS) against this kernel with beam = inf and max_active =
    Q + A (the state in global memory).  The two must agree within the header's tolerances; asserted.

Timed with HIP events alone, median of 5 calls after a warm-up call, three runs (the machine is shared), the middle one
reported; both sides of a comparison in the same process.  One JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_graph_beam_bench as BB  # noqa: E402
import ctc_graph_decode_bench as DB  # noqa: E402
import ctc_graph_logp_bench as LB  # noqa: E402
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import DecodingGraph, GraphSet  # noqa: E402

DEV = "cuda"
INF = float("inf")


class Run:
    """Score and gradient calls of the pruned sum on one batch, their buffers allocated once."""

    def __init__(self, logits, graph, beam, max_active=None):
        B, T, V = logits.shape
        self.lib = hip.lib()
        self.g = hip.beam_logp_graph(graph, DEV)
        U, Q, A = len(graph.cols), graph.num_nodes, graph.num_arcs
        max_active = Q + A if max_active is None else max_active
        self.bytes = (self.lib.oe_ctc_graph_beam_logp_workspace_bytes(B, T, U, Q, A, max_active),
                      self.lib.oe_ctc_graph_beam_logp_grad_workspace_bytes(B, T, U, Q, A, max_active))
        assert min(self.bytes) > 0
        self.ws = [torch.empty(n, dtype=torch.uint8, device=DEV) for n in self.bytes]
        self.hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        self.w = torch.ones(B, device=DEV)
        self.logp, self.dl, self.logits = torch.empty(B, device=DEV), torch.empty(B, T, V, device=DEV), logits
        self.status, self.peak = torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
        self.s, self.gr = hip.CtcGraphBeamLogpArgs(), hip.CtcGraphBeamLogpGradArgs()
        for a in (self.s, self.gr):
            a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, self.hl.data_ptr()
            a.graph, a.normalized, a.max_active, a.beam = C.pointer(self.g), 0, max_active, beam
            a.logp, a.status, a.peak = self.logp.data_ptr(), self.status.data_ptr(), self.peak.data_ptr()
        self.s.workspace = self.ws[0].data_ptr()
        self.gr.workspace, self.gr.g, self.gr.dlogits = self.ws[1].data_ptr(), self.w.data_ptr(), self.dl.data_ptr()

    def score(self):
        hip.check(self.lib.oe_ctc_graph_beam_logp(C.byref(self.s), hip.stream()), "oe_ctc_graph_beam_logp")

    def grad(self):
        hip.check(self.lib.oe_ctc_graph_beam_logp_grad(C.byref(self.gr), hip.stream()), "oe_ctc_graph_beam_logp_grad")

    def times(self, T):
        ms_s, runs_s = BB.middle(self.score)
        ms_g, runs_g = BB.middle(self.grad)
        return {"score_ms": ms_s, "score_runs_ms": runs_s, "grad_ms": ms_g, "grad_runs_ms": runs_g,
                "score_us_per_frame": round(ms_s * 1e3 / T, 2), "grad_us_per_frame": round(ms_g * 1e3 / T, 2),
                "workspace_MiB": [round(n / 2 ** 20, 1) for n in self.bytes]}


def lexicon(n_words=100_000, beams=(12.0, 8.0), max_active=1 << 17):
    B, T = 8, 120
    ph = BB.words(13, n_words, 2, 4, BB.V_LEX)
    rng = np.random.default_rng(17)
    graph = DecodingGraph.from_phrases(ph, weights=(-3.0 * rng.random(n_words)).tolist(), loop=True, large=True)
    logits = BB.planted(ph, B, T, 19, BB.V_LEX)
    rows = []
    for beam in beams:
        best = BB.Run(logits, graph, beam, max_active)
        b = best.results()
        ms_b, runs_b = BB.middle(best)
        del best
        run = Run(logits, graph, beam, max_active)
        run.score()
        run.grad()
        torch.cuda.synchronize()
        assert run.status.tolist() == b[9].tolist() == [0] * B, (run.status.tolist(), b[9].tolist())
        assert bool((run.logp.cpu() >= torch.from_numpy(b[0]) - 1e-3).all()), "the pruned sum is below the best path's score"
        row = {"beam": beam, "max_active": max_active, "oe_ctc_graph_beam_ms": ms_b, "oe_ctc_graph_beam_runs_ms": runs_b,
               "peak_max": int(b[10].max()), "peak_sum": int(run.peak.max()), **run.times(T)}
        row["score_over_max"] = round(row["score_ms"] / ms_b, 2)
        row["grad_over_max"] = round(row["grad_ms"] / ms_b, 2)
        rows.append(row)
        del run
    return {"words": n_words, "V": BB.V_LEX, "Q": graph.num_nodes, "A": graph.num_arcs, "U": len(graph.cols), "B": B, "T": T, "rows": rows}


def at_the_dense_limits():
    DB.K = LB.K
    ph = DB.phrases(7)
    logits, _ = DB.planted(ph, 11)
    graph = DecodingGraph.from_phrases(ph, loop=True)
    dense = LB.Run(logits, GraphSet([graph]))
    dense.score()
    dense.grad()
    run = Run(logits, graph, INF)
    run.score()
    run.grad()
    torch.cuda.synchronize()
    err = (run.logp - dense.logp).abs() / (1e-3 + 1e-4 * dense.logp.abs())
    gerr = (run.dl - dense.dl).abs() / (2e-5 + 2e-3 * dense.dl.abs())
    assert float(err.max()) <= 1 and float(gerr.max()) <= 1, (float(err.max()), float(gerr.max()))
    d, p = dense.times(), run.times(LB.T)
    return {"graph": "trie_loop", "Q": graph.num_nodes, "A": graph.num_arcs, "U": len(graph.cols), "B": LB.B, "T": LB.T, "V": LB.V,
            "oe_ctc_graph_logp": d, "oe_ctc_graph_beam_logp_inf": p, "tolerance_fraction": [round(float(err.max()), 4), round(float(gerr.max()), 4)],
            "score_over_dense": round(p["score_ms"] / d["score_ms"], 2), "grad_over_dense": round(p["grad_ms"] / d["grad_ms"], 2)}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_graph_beam_logp_bench needs a GPU"
    res = {"bench": "ctc_graph_beam_logp", "device": torch.cuda.get_device_name(0), "lexicon": lexicon(),
           "at_the_dense_limits": at_the_dense_limits()}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
