#!/usr/bin/env python3
"""The graph CTC likelihood and its gradient on the device (oe_ctc_graph_logp / oe_ctc_graph_logp_grad) at the size of their
users (GPU box).

  python tools/ctc_graph_logp_bench.py [--out FILE]

One shape, B = 32 utterances of T = 250 frames, V = 4233 (tools/ctc_graph_decode_bench.py's), synthetic logits with a planted
labelling that speaks phrases of the list:
  (a) linear      a chain per utterance (its planted tokens; a set of B graphs) against oe_ctc_nbest_score + oe_ctc_nbest_grad
                  with group 1: the same mathematics in the n-best scorer's form (a lane per state, neighbours by DPP);
  (b) trie_loop   800 phrases of 6 labels as a looped prefix trie (the likelihood kernel holds 5120 arcs, so not the decode
                  bench's 1000), and token_loop, one node and V - 1 self-loops, against oe_ctc_graph (Viterbi) on the same
                  graph.
The calls are checked at the size they are timed at: (a) must agree with the n-best scorer within the header's tolerances, the
token loop must give logp = 0 and a zero gradient, and logp >= the Viterbi score everywhere.

Timed with HIP events alone, median of 5 calls after a warm-up call, three runs (the machine is shared), the middle one
reported.  One JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_graph_decode_bench as DB  # noqa: E402
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import DecodingGraph, GraphSet  # noqa: E402

DEV = "cuda"
B, T, V, L = DB.B, DB.T, DB.V, DB.L
K = 800


class Run:
    """Score and gradient calls on one batch with their buffers."""

    def __init__(self, logits, gset, graph_of=None):
        self.lib, self.gset = hip.lib(), gset
        self.set = hip.graph_set(gset, DEV)
        U = len(gset.cols)
        self.bytes = (self.lib.oe_ctc_graph_logp_workspace_bytes(B, T, U, gset.Qmax, gset.Amax),
                      self.lib.oe_ctc_graph_logp_grad_workspace_bytes(B, T, U, gset.Qmax, gset.Amax))
        assert min(self.bytes) > 0
        self.ws = [torch.empty(n, dtype=torch.uint8, device=DEV) for n in self.bytes]
        self.hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        self.of = None if graph_of is None else torch.as_tensor(graph_of, dtype=torch.int32).to(DEV)
        self.g = torch.ones(B, device=DEV)
        self.logp, self.dl, self.logits = torch.empty(B, device=DEV), torch.empty(B, T, V, device=DEV), logits
        s, g = self.s, self.gr = hip.CtcGraphLogpArgs(), hip.CtcGraphLogpGradArgs()
        for a in (s, g):
            a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, self.hl.data_ptr()
            a.set, a.graph_of, a.normalized = C.pointer(self.set), (None if self.of is None else self.of.data_ptr()), 0
            a.logp = self.logp.data_ptr()
        s.workspace = self.ws[0].data_ptr()
        g.workspace, g.g, g.dlogits = self.ws[1].data_ptr(), self.g.data_ptr(), self.dl.data_ptr()

    def score(self):
        hip.check(self.lib.oe_ctc_graph_logp(C.byref(self.s), hip.stream()), "oe_ctc_graph_logp")

    def grad(self):
        hip.check(self.lib.oe_ctc_graph_logp_grad(C.byref(self.gr), hip.stream()), "oe_ctc_graph_logp_grad")

    def times(self):
        ms_s, runs_s = DB.middle(self.score)
        ms_g, runs_g = DB.middle(self.grad)
        return {"score_ms": round(ms_s, 3), "score_runs_ms": runs_s, "grad_ms": round(ms_g, 3), "grad_runs_ms": runs_g,
                "score_us_per_frame": round(ms_s * 1e3 / T, 2), "grad_us_per_frame": round(ms_g * 1e3 / T, 2),
                "workspace_MiB": [round(n / 2 ** 20, 1) for n in self.bytes]}


def nbest(logits, tokens):
    """oe_ctc_nbest_score (with `saved`) + oe_ctc_nbest_grad, group 1, on the planted tokens."""
    lib = hip.lib()
    Lmax = max(len(y) for y in tokens)
    assert Lmax <= 255
    ys = torch.zeros(B, Lmax, dtype=torch.int32)
    for b, y in enumerate(tokens):
        ys[b, :len(y)] = torch.tensor(y, dtype=torch.int32)
    ys, yl = ys.to(DEV), torch.tensor([len(y) for y in tokens], dtype=torch.int32, device=DEV)
    hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.oe_ctc_nbest_workspace_bytes(B, T, 1, Lmax), dtype=torch.uint8, device=DEV)
    saved = torch.empty(lib.oe_ctc_nbest_saved_bytes(B, T, 1, Lmax), dtype=torch.uint8, device=DEV)
    logp, g, dl = torch.empty(B, device=DEV), torch.ones(B, device=DEV), torch.empty(B, T, V, device=DEV)

    def score():
        hip.call("oe_ctc_nbest_score", logits, V, B, T, V, hl, ys, Lmax, yl, 1, Lmax, logp, saved, ws)

    def both():
        score()
        hip.call("oe_ctc_nbest_grad", logits, V, B, T, V, hl, ys, Lmax, yl, 1, Lmax, logp, g, saved, dl, None)

    both()
    torch.cuda.synchronize()
    ms_s, runs_s = DB.middle(score)
    ms_b, runs_b = DB.middle(both)
    return logp, dl, {"labels": [int(yl.min()), int(yl.max())], "score_ms": round(ms_s, 3), "score_runs_ms": runs_s,
                      "score_and_grad_ms": round(ms_b, 3), "score_and_grad_runs_ms": runs_b}


def viterbi(logits, graph):
    run = DB.Run(logits, graph)
    run()
    torch.cuda.synchronize()
    ms, runs = DB.middle(run)
    return run.keep[2].clone(), {"call_ms": round(ms, 3), "call_runs_ms": runs}


def part(name, logits, graph):
    run = Run(logits, GraphSet([graph]))
    run.score()
    run.grad()
    torch.cuda.synchronize()
    best, vit = viterbi(logits, graph)
    assert bool((run.logp >= best - 1e-3).all()), f"{name}: the likelihood is below the best path's score"
    out = {"graph": name, "Q": graph.num_nodes, "A": graph.num_arcs, "U": len(graph.cols), **run.times(), "oe_ctc_graph": vit}
    out["score_over_viterbi"] = round(out["score_ms"] / vit["call_ms"], 2)
    out["grad_over_viterbi"] = round(out["grad_ms"] / vit["call_ms"], 2)
    return out, run


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_graph_logp_bench needs a GPU"
    DB.K = K
    ph = DB.phrases(7)
    logits, tokens = DB.planted(ph, 11)
    # (a) linear chains against the n-best scorer
    run = Run(logits, GraphSet([DecodingGraph.linear(y) for y in tokens]), graph_of=np.arange(B))
    run.score()
    run.grad()
    nb_logp, nb_dl, nb = nbest(logits, tokens)
    torch.cuda.synchronize()
    err = (run.logp - nb_logp).abs() / (1e-3 + 1e-4 * nb_logp.abs())
    gerr = (run.dl - nb_dl).abs() / (2e-5 + 2e-3 * nb_dl.abs())
    assert float(err.max()) <= 1 and float(gerr.max()) <= 1, (float(err.max()), float(gerr.max()))
    linear = {"graph": "linear", "Qmax": run.gset.Qmax, "Amax": run.gset.Amax, "U": len(run.gset.cols), **run.times(), "oe_ctc_nbest": nb,
              "tolerance_fraction": [round(float(err.max()), 4), round(float(gerr.max()), 4)]}
    linear["score_over_nbest"] = round(linear["score_ms"] / nb["score_ms"], 2)
    linear["grad_over_nbest"] = round(linear["grad_ms"] / nb["score_and_grad_ms"], 2)
    # (b) a looped trie and a token loop against the Viterbi kernel
    trie, _ = part("trie_loop", logits, DecodingGraph.from_phrases(ph, loop=True))
    loop, lrun = part("token_loop", logits, DecodingGraph.token_loop(V))
    assert float(lrun.logp.abs().max()) <= 1e-3 and float(lrun.dl.abs().max()) <= 2e-5, "token loop: logp and gradient must vanish"
    res = {"bench": "ctc_graph_logp", "device": torch.cuda.get_device_name(0), "B": B, "T": T, "V": V, "phrases": K, "labels_per_phrase": L,
           "graphs": [linear, trie, loop]}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
