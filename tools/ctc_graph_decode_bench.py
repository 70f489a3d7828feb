#!/usr/bin/env python3
"""Grammar-constrained CTC decoding on the device (oe_ctc_graph) at the size of its users (GPU box).

  python tools/ctc_graph_decode_bench.py [--out FILE]

One shape, B = 32 utterances of T = 250 frames, V = 4233, three graphs:
  token_loop   one node, V - 1 self-loops: unconstrained best-path decoding
  trie         1000 phrases of 6 random labels as a prefix trie
  trie_loop    the same trie with every phrase returning to the start: sequences of phrases
Synthetic logits: randn with +14 on a planted frame labelling that speaks phrases of the list with blanks between them, so the
call is also checked at the size it is timed at: token_loop and trie_loop must return the planted tokens.

Timed with HIP events alone, median of 5 calls after a warm-up call, three runs (the machine is shared), the middle one
reported.  Launch 1 is oe_ctc_kws's (lp_rows_kernel, one kernel for both), so it is timed through oe_ctc_kws with the graph's columns and
every keyword empty (its launch 2 then only writes empty results); launch 2 is the full call minus that.  `floor` is launch 2
on a graph of one self-loop with the same columns: Tb frames of two barriers each and the fixed parts (end arg-max,
back-trace, traversal scan) with next to no state to update.  oe_ctc_align on the same logits, each utterance aligned to its
planted tokens, stands beside them.  One JSON line."""
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
from openeat_amd.utils.keyword import KeywordList  # noqa: E402

DEV = "cuda"
B, T, V, K, L = 32, 250, 4233, 1000, 6


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
    return sorted(runs)[1], [round(x, 3) for x in runs]


def phrases(seed):
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < K:
        y = tuple(int(c) for c in 1 + np.cumsum(rng.integers(1, V - 1, size=L)) % (V - 1))
        if y not in seen:                               # never the same label twice in a row
            seen.add(y)
            out.append(y)
    return out


def planted(ph, seed):
    """-> logits (B, T, V) on the device and the planted tokens per utterance: phrases of the list, two frames a label, blanks between."""
    rng = np.random.default_rng(seed)
    path = np.zeros((B, T), dtype=np.int64)
    tokens = []
    for b in range(B):
        t, toks = int(rng.integers(1, 6)), []
        while t + 2 * L + 2 < T:
            y = ph[int(rng.integers(0, K))]
            for c in y:
                path[b, t: t + 2] = c
                t += 2
            toks += list(y)
            t += int(rng.integers(2, 8))
        tokens.append(toks)
    g = torch.Generator(device=DEV).manual_seed(seed)
    logits = torch.randn(B, T, V, device=DEV, generator=g)
    logits.scatter_add_(2, torch.from_numpy(path).to(DEV)[:, :, None], torch.full((B, T, 1), 14.0, device=DEV))
    return logits, tokens


class Run:
    def __init__(self, logits, graph):
        self.lib, self.graph = hip.lib(), graph
        self.g = hip.decoding_graph(graph, DEV)
        self.nbytes = self.lib.oe_ctc_graph_workspace_bytes(B, T, len(graph.cols), graph.num_nodes, graph.num_arcs)
        assert self.nbytes > 0
        self.keep = [torch.empty(self.nbytes, dtype=torch.uint8, device=DEV), torch.full((B,), T, dtype=torch.int32, device=DEV),
                     torch.empty(B, device=DEV), torch.empty(B, T, dtype=torch.int32, device=DEV), torch.empty(B, T, dtype=torch.int32, device=DEV),
                     torch.empty(B, T, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)]
        self.keep += [torch.empty(B, T, dtype=torch.int32, device=DEV) for _ in range(3)] + [torch.empty(B, T, device=DEV), logits]
        ws, hl, score, frames, arcs, plp, n_trav, ta, ts, te, tl, _ = self.keep
        a = self.a = hip.CtcGraphArgs()
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, hl.data_ptr()
        a.graph, a.normalized, a.max_trav, a.workspace = C.pointer(self.g), 0, T, ws.data_ptr()
        a.score, a.frames, a.arcs, a.path_logp = score.data_ptr(), frames.data_ptr(), arcs.data_ptr(), plp.data_ptr()
        a.n_trav, a.trav_arc, a.trav_start, a.trav_end, a.trav_logp = n_trav.data_ptr(), ta.data_ptr(), ts.data_ptr(), te.data_ptr(), tl.data_ptr()

    def __call__(self):
        hip.check(self.lib.oe_ctc_graph(C.byref(self.a), hip.stream()), "oe_ctc_graph")

    def tokens(self):
        torch.cuda.synchronize()
        n, ta = self.keep[6].cpu().numpy(), self.keep[7].cpu().numpy()
        return [self.graph.label[ta[b, : n[b]]].tolist() for b in range(B)], self.keep[2].cpu().numpy()


def rows_alone(logits, cols):
    """launch 1 alone: oe_ctc_kws over the same columns with every keyword empty."""
    kl = KeywordList([[int(c)] for c in cols])
    Kc = len(kl)
    q = hip.keyword_set(kl, DEV)
    zero = torch.zeros(Kc, dtype=torch.int32, device=DEV)
    q.klens = zero.data_ptr()
    lib = hip.lib()
    keep = [torch.empty(lib.oe_ctc_kws_workspace_bytes(B, T, len(cols)), dtype=torch.uint8, device=DEV),
            torch.full((B,), T, dtype=torch.int32, device=DEV), torch.empty(B, Kc, dtype=torch.int32, device=DEV)]
    keep += [torch.empty(B, Kc, 1, dtype=torch.int32, device=DEV) for _ in range(2)] + [torch.empty(B, Kc, 1, device=DEV), zero, logits]
    a = hip.CtcKwsArgs()
    a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, keep[1].data_ptr()
    a.kws, a.normalized, a.max_hits, a.workspace = C.pointer(q), 0, 1, keep[0].data_ptr()
    a.n_hits, a.hit_start, a.hit_end, a.hit_score = (t.data_ptr() for t in keep[2:6])
    return middle(lambda: hip.check(lib.oe_ctc_kws(C.byref(a), hip.stream()), "oe_ctc_kws"))


def one_loop(graph):
    """A graph of one self-loop that keeps `graph`'s columns: launch 1 does the same work, launch 2 next to none per frame."""
    g = DecodingGraph(1, [(0, 0, int(graph.cols[0]), 0.0)], {0: 0.0})
    g.cols = graph.cols.copy()
    return g


def part(name, logits, graph, want_tokens):
    run = Run(logits, graph)
    run()
    toks, score = run.tokens()
    assert np.isfinite(score).all(), f"{name}: an utterance is infeasible"
    if want_tokens is not None:
        bad = [b for b in range(B) if toks[b] != want_tokens[b]]
        assert not bad, f"{name}: utterances {bad[:5]} did not decode to the planted tokens"
    ms_all, runs_all = middle(run)
    ms_rows, runs_rows = rows_alone(logits, graph.cols)
    ms_floor, _ = middle(Run(logits, one_loop(graph)))
    return {"graph": name, "Q": graph.num_nodes, "A": graph.num_arcs, "U": len(graph.cols), "max_in_degree": int(np.diff(graph.in_ptr).max()),
            "workspace_MiB": round(run.nbytes / 2 ** 20, 1), "call_ms": round(ms_all, 3), "call_runs_ms": runs_all,
            "launch1_ms": round(ms_rows, 3), "launch1_runs_ms": runs_rows, "launch2_ms": round(ms_all - ms_rows, 3),
            "launch2_us_per_frame": round((ms_all - ms_rows) * 1e3 / T, 2), "launch2_floor_ms": round(ms_floor - ms_rows, 3),
            "back_pointer_MiB": round(4 * B * T * (graph.num_nodes + (graph.num_arcs + 3) // 4) / 2 ** 20, 1)}


def align(logits, tokens):
    Lmax = max(len(y) for y in tokens)
    ys = torch.zeros(B, Lmax, dtype=torch.int32)
    for b, y in enumerate(tokens):
        ys[b, : len(y)] = torch.tensor(y, dtype=torch.int32)
    ys, yl = ys.to(DEV), torch.tensor([len(y) for y in tokens], dtype=torch.int32, device=DEV)
    hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    frames, score = torch.empty(B, T, dtype=torch.int32, device=DEV), torch.empty(B, device=DEV)
    ws = torch.empty(hip.lib().oe_ctc_align_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=DEV)
    ms, runs = middle(lambda: hip.call("oe_ctc_align", logits, V, B, T, V, hl, ys, Lmax, yl, frames, None, None, None, score, ws))
    return {"labels": [int(yl.min()), int(yl.max())], "call_ms": round(ms, 3), "call_runs_ms": runs}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_graph_decode_bench needs a GPU"
    ph = phrases(7)
    logits, tokens = planted(ph, 11)
    res = {"bench": "ctc_graph", "device": torch.cuda.get_device_name(0), "B": B, "T": T, "V": V, "phrases": K, "labels_per_phrase": L,
           "graphs": [part("token_loop", logits, DecodingGraph.token_loop(V), tokens),
                      part("trie", logits, DecodingGraph.from_phrases(ph), None),
                      part("trie_loop", logits, DecodingGraph.from_phrases(ph, loop=True), tokens)],
           "oe_ctc_align": align(logits, tokens)}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
