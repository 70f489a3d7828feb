#!/usr/bin/env python3
"""Beam-pruned CTC decoding over large token graphs (oe_ctc_graph_beam) beside the dense kernel and at the size it was built
for (GPU box).  Synthetic data, no downloads.

  python tools/ctc_graph_beam_bench.py [--out FILE]

(a) in_limit: the looped trie of 1000 six-label phrases of tools/ctc_graph_decode_bench.py, B = 32 x T = 250, V = 4233:
    oe_ctc_graph against oe_ctc_graph_beam with beam = inf and max_active = Q + A.  The outputs must be equal; the ratio says
    what token passing in global memory costs where the dense kernel's LDS would have done.
(b) lexicon: a loop of 100 000 words of two to four tokens over 1999 tokens with a unigram weight each (the output may only
    contain in-vocabulary words), B = 8 x T = 120, V = 2000, on peaked posteriors (randn + 14 on a planted labelling that speaks
    words of the lexicon): beam = inf with max_active = Q + A, then three finite beams with max_active = 2^17: ms per batch, the
    largest peak, and the share of utterances whose frame labelling equals the unpruned one.  (The last frame is not pruned,
    so while node 0 is alive a peak is at least the number of first tokens: hence fewer tokens than in (a).)
(c) the relation that must hold: a finite beam whose peak stays under 1 % of Q + A runs faster than beam = inf on the same input
    (the per-frame cost follows the active set, not the graph).  Asserted.

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
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import DecodingGraph  # noqa: E402

DEV = "cuda"
V, V_LEX = 4233, 2000
INF = float("inf")


def timed(fn, n=5, warm=1):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(n + warm):
        if i >= warm:
            ev[i - warm][0].record()
        fn()
        if i >= warm:
            ev[i - warm][1].record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[n // 2]


def middle(fn):
    runs = [timed(fn) for _ in range(3)]
    return round(sorted(runs)[1], 3), [round(x, 3) for x in runs]


def words(seed, count, lo, hi, V=V):
    """`count` distinct token sequences of lo .. hi labels, never the same label twice in a row."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < count:
        y = tuple(int(c) for c in 1 + np.cumsum(rng.integers(1, V - 1, size=int(rng.integers(lo, hi + 1)))) % (V - 1))
        if y not in seen:
            seen.add(y)
            out.append(y)
    return out


def planted(ph, B, T, seed, V=V):
    """logits (B, T, V) on the device: randn with +14 on a frame labelling that speaks phrases of `ph`, two frames a label."""
    rng = np.random.default_rng(seed)
    path = np.zeros((B, T), dtype=np.int64)
    longest = max(len(y) for y in ph)
    for b in range(B):
        t = int(rng.integers(1, 6))
        while t + 2 * longest + 2 < T:
            for c in ph[int(rng.integers(0, len(ph)))]:
                path[b, t: t + 2] = c
                t += 2
            t += int(rng.integers(2, 8))
    g = torch.Generator(device=DEV).manual_seed(seed)
    logits = torch.randn(B, T, V, device=DEV, generator=g)
    logits.scatter_add_(2, torch.from_numpy(path).to(DEV)[:, :, None], torch.full((B, T, 1), 14.0, device=DEV))
    return logits


class Run:
    """One prepared call of oe_ctc_graph (beam None) or oe_ctc_graph_beam, its buffers allocated once."""

    def __init__(self, logits, graph, beam=None, max_active=None):
        B, T, V = logits.shape
        self.lib, self.beam = hip.lib(), beam
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)
        self.hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        self.out = [f32(B), i32(B, T), i32(B, T), f32(B, T), i32(B), i32(B, T), i32(B, T), i32(B, T), f32(B, T), i32(B), i32(B)]
        U, Q, A = len(graph.cols), graph.num_nodes, graph.num_arcs
        if beam is None:
            self.g, a = hip.decoding_graph(graph, DEV), hip.CtcGraphArgs()
            self.nbytes, self.fn = self.lib.oe_ctc_graph_workspace_bytes(B, T, U, Q, A), self.lib.oe_ctc_graph
        else:
            self.g, a = hip.beam_graph(graph, DEV), hip.CtcGraphBeamArgs()
            a.max_active, a.beam = (Q + A if max_active is None else max_active), beam
            self.nbytes, self.fn = self.lib.oe_ctc_graph_beam_workspace_bytes(B, T, U, Q, A, a.max_active), self.lib.oe_ctc_graph_beam
            a.status, a.peak = self.out[9].data_ptr(), self.out[10].data_ptr()
        assert self.nbytes > 0
        self.ws, self.logits, self.a = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV), logits, a
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, self.hl.data_ptr()
        a.graph, a.normalized, a.max_trav, a.workspace = C.pointer(self.g), 0, T, self.ws.data_ptr()
        (a.score, a.frames, a.arcs, a.path_logp, a.n_trav, a.trav_arc, a.trav_start, a.trav_end, a.trav_logp) = (t.data_ptr() for t in self.out[:9])

    def __call__(self):
        hip.check(self.fn(C.byref(self.a), hip.stream()), "oe_ctc_graph" if self.beam is None else "oe_ctc_graph_beam")

    def results(self):
        self()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.out]


def in_limit():
    B, T = 32, 250
    ph = words(7, 1000, 6, 6)
    graph = DecodingGraph.from_phrases(ph, loop=True)
    logits = planted(ph, B, T, 11)
    dense, beam = Run(logits, graph), Run(logits, graph, INF)
    d, b = dense.results(), beam.results()
    assert np.isfinite(d[0]).all() and all(np.array_equal(x, y) for x, y in zip(d[:9], b[:9])), "the beam kernel without a beam differs from oe_ctc_graph"
    ms_d, runs_d = middle(dense)
    ms_b, runs_b = middle(beam)
    return {"Q": graph.num_nodes, "A": graph.num_arcs, "B": B, "T": T, "dense_ms": ms_d, "dense_runs_ms": runs_d, "beam_inf_ms": ms_b,
            "beam_inf_runs_ms": runs_b, "beam_inf_over_dense": round(ms_b / ms_d, 2), "peak": int(b[10].max()),
            "dense_workspace_MiB": round(dense.nbytes / 2 ** 20, 1), "beam_workspace_MiB": round(beam.nbytes / 2 ** 20, 1)}


def lexicon(n_words=100_000, beams=(12.0, 8.0, 4.0), max_active=1 << 17):
    B, T = 8, 120
    ph = words(13, n_words, 2, 4, V_LEX)
    rng = np.random.default_rng(17)
    graph = DecodingGraph.from_phrases(ph, weights=(-3.0 * rng.random(n_words)).tolist(), loop=True, large=True)
    logits = planted(ph, B, T, 19, V_LEX)
    states = graph.num_nodes + graph.num_arcs
    free = Run(logits, graph, INF)
    f = free.results()
    assert (f[9] == 0).all(), "an utterance is infeasible without a beam"
    ms, runs = middle(free)
    rows = [{"beam": "inf", "max_active": states, "ms": ms, "runs_ms": runs, "peak": int(f[10].max()), "same_path": 1.0,
             "workspace_MiB": round(free.nbytes / 2 ** 20, 1)}]
    del free
    for beam in beams:
        run = Run(logits, graph, beam, max_active)
        r = run.results()
        ms, runs = middle(run)
        same = float(np.mean([r[9][b] == 0 and np.array_equal(r[1][b], f[1][b]) for b in range(B)]))
        rows.append({"beam": beam, "max_active": max_active, "ms": ms, "runs_ms": runs, "peak": int(r[10].max()), "same_path": round(same, 3),
                     "status": sorted(set(r[9].tolist())), "workspace_MiB": round(run.nbytes / 2 ** 20, 1)})
    small = [r for r in rows[1:] if r["peak"] < states // 100 and r["status"] == [0]]
    holds = bool(small) and all(r["ms"] < rows[0]["ms"] for r in small)
    return {"words": n_words, "V": V_LEX, "Q": graph.num_nodes, "A": graph.num_arcs, "U": len(graph.cols), "B": B, "T": T, "rows": rows,
            "beams_under_1_percent": [r["beam"] for r in small], "finite_beam_faster_than_inf": holds}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_graph_beam_bench needs a GPU"
    res = {"bench": "ctc_graph_beam", "device": torch.cuda.get_device_name(0), "V": V, "in_limit": in_limit(), "lexicon": lexicon()}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    assert res["lexicon"]["finite_beam_faster_than_inf"], "a finite beam that keeps peak under 1 % of Q + A must run faster than beam = inf"
