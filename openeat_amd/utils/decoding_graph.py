"""Host side of grammar-constrained CTC decoding (ASRModel.ctc_graph_search, ops.ctc_graph_decode; semantics in
include/openeat_hip.h, oe_ctc_graph): the token graph with the tables the kernel reads, its builders, and the records made of
the kernel's outputs.  No kernel here."""
import math
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

MAX_NODES = 8064                 # OE_CTC_GRAPH_MAX_NODES: 12 bytes of LDS per node
MAX_ARCS = 16384                 # OE_CTC_GRAPH_MAX_ARCS: 4 bytes of LDS per arc
NEG_INF = float("-inf")


class DecodingGraph:
    """DecodingGraph(num_nodes, arcs, finals, outputs=None): an epsilon-free weighted token graph.  Node 0 is the start.
    arcs = (src, dst, label, weight) each, label a token id >= 1 (blank, 0, is never a label), weight a finite natural log;
    finals = {node: weight} or one weight per node with -inf for "not final"; outputs = per arc, in the caller's order, what a
    traversal of the arc emits (a word, a phrase index, anything) or None.  The graph may be non-deterministic and may have
    self-loops, parallel arcs and unreachable nodes.

    Arcs are kept sorted by dst, stable: within a node the caller's order stays, and an arc's id is its position in that order
    (`order[id]` = the caller's index, `arc_id[caller's index]` = id).  Host tables (oe_decoding_graph): in_ptr (Q+1) int32, the
    arcs into q are in_ptr[q] .. in_ptr[q+1]-1; src, dst, label (A) int32; cols (U) int32 = the distinct labels, ascending;
    col (A) int32 = the index of label into cols; w (A) float32; final (Q) float32."""

    def __init__(self, num_nodes: int, arcs: Sequence[Sequence], finals, outputs: Optional[Sequence] = None):
        Q = int(num_nodes)
        if not 1 <= Q <= MAX_NODES:
            raise ValueError(f"DecodingGraph: {Q} nodes outside 1 .. {MAX_NODES}")
        arcs = [tuple(a) for a in arcs]
        A = len(arcs)
        if A > MAX_ARCS:
            raise ValueError(f"DecodingGraph: {A} arcs exceed {MAX_ARCS}")
        for a in arcs:
            if len(a) != 4:
                raise ValueError(f"DecodingGraph: an arc is (src, dst, label, weight), got {a}")
            s, d, lab, wt = a
            if not (0 <= int(s) < Q and 0 <= int(d) < Q):
                raise ValueError(f"DecodingGraph: arc {a} leaves the nodes 0 .. {Q - 1}")
            if int(lab) != lab or int(lab) < 1:
                raise ValueError(f"DecodingGraph: arc {a}: a label is a token id >= 1 (0 is the blank; there are no epsilon arcs)")
            if not math.isfinite(float(wt)):
                raise ValueError(f"DecodingGraph: arc {a}: a weight is finite")
        if isinstance(finals, dict):
            fin = np.full(Q, -np.inf, dtype=np.float32)
            for q, wt in finals.items():
                if not 0 <= int(q) < Q:
                    raise ValueError(f"DecodingGraph: final node {q} outside 0 .. {Q - 1}")
                fin[int(q)] = wt
        else:
            fin = np.asarray(list(finals), dtype=np.float32)
            if fin.shape != (Q,):
                raise ValueError(f"DecodingGraph: finals is a dict or one weight per node ({Q}), got {fin.shape}")
        if np.isnan(fin).any() or np.isposinf(fin).any():
            raise ValueError("DecodingGraph: a final weight is finite, or -inf for a node that is not final")
        if outputs is not None and len(outputs) != A:
            raise ValueError(f"DecodingGraph: one output per arc ({A}), got {len(outputs)}")
        self.num_nodes, self.num_arcs = Q, A
        order = sorted(range(A), key=lambda i: int(arcs[i][1]))        # sorted() is stable
        self.order = np.asarray(order, dtype=np.int32).reshape(A)
        self.arc_id = np.empty(A, dtype=np.int32)
        self.arc_id[self.order] = np.arange(A, dtype=np.int32)
        self.src = np.asarray([int(arcs[i][0]) for i in order], dtype=np.int32).reshape(A)
        self.dst = np.asarray([int(arcs[i][1]) for i in order], dtype=np.int32).reshape(A)
        self.label = np.asarray([int(arcs[i][2]) for i in order], dtype=np.int32).reshape(A)
        self.w = np.asarray([float(arcs[i][3]) for i in order], dtype=np.float32).reshape(A)
        self.final = fin
        self.outputs = [None] * A if outputs is None else [outputs[i] for i in order]
        self.in_ptr = np.zeros(Q + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.dst, minlength=Q), out=self.in_ptr[1:])
        self.cols = np.unique(self.label).astype(np.int32)
        self.col = np.searchsorted(self.cols, self.label).astype(np.int32)
        self.skipped = 0
        self._device: Dict[object, tuple] = {}

    # ---- builders ---------------------------------------------------------------------------------------------------
    @classmethod
    def linear(cls, tokens: Sequence[int]) -> "DecodingGraph":
        """The chain that accepts `tokens` alone, weights 0: oe_ctc_align's problem, ties included."""
        toks = [int(t) for t in tokens]
        return cls(len(toks) + 1, [(i, i + 1, t, 0.0) for i, t in enumerate(toks)], {len(toks): 0.0})

    @classmethod
    def from_phrases(cls, phrases: Sequence[Sequence[int]], weights: Optional[Sequence[float]] = None,
                     outputs: Optional[Sequence] = None, loop: bool = False) -> "DecodingGraph":
        """A prefix trie over the phrases (token-id sequences of at least one label, no two alike).  All but a phrase's last
        token share the trie's arcs; its last arc is its own - it carries weights[i] (default 0) and outputs[i] (default i)
        and ends in a final node of its own, so a phrase that is the beginning of another emits only its own output.
        loop=True: the last arc returns to node 0, which is final, so sequences of phrases decode without epsilons."""
        phrases = [tuple(int(t) for t in p) for p in phrases]
        if not phrases or any(len(p) == 0 for p in phrases):
            raise ValueError("DecodingGraph.from_phrases: at least one phrase, each of at least one token")
        if len(set(phrases)) != len(phrases):
            raise ValueError("DecodingGraph.from_phrases: a phrase is listed twice")
        wts = [0.0] * len(phrases) if weights is None else [float(x) for x in weights]
        outs = list(range(len(phrases))) if outputs is None else list(outputs)
        if len(wts) != len(phrases) or len(outs) != len(phrases):
            raise ValueError("DecodingGraph.from_phrases: one weight and one output per phrase")
        arcs, arc_out, finals, child, n = [], [], {}, {}, 1
        for p, wt, out in zip(phrases, wts, outs):
            q = 0
            for t in p[:-1]:
                nxt = child.get((q, t))
                if nxt is None:
                    nxt = child[(q, t)] = n
                    n += 1
                    arcs.append((q, nxt, t, 0.0))
                    arc_out.append(None)
                q = nxt
            if loop:
                end = 0
            else:
                end = n
                n += 1
            arcs.append((q, end, p[-1], wt))
            arc_out.append(out)
            finals[end] = 0.0
        return cls(n, arcs, finals, arc_out)

    @classmethod
    def from_text(cls, lines: Iterable[str], token2id, weights: Optional[Sequence[float]] = None, loop: bool = False) -> "DecodingGraph":
        """One phrase per line, split into the recipe's character tokens (every non-space character, as
        KeywordList.from_text); a phrase's output is its text.  A line with a character token2id does not list (or maps to the
        blank) is skipped and counted in `.skipped`; empty lines and repeated phrases (the first is kept) are dropped.
        weights: one per line of `lines`."""
        phrases, texts, wts, seen, skipped = [], [], [], set(), 0
        for i, line in enumerate(lines):
            chars = [ch for ch in line if not ch.isspace()]
            if not chars:
                continue
            ids = tuple(token2id.get(ch, 0) for ch in chars)
            if any(t <= 0 for t in ids):
                skipped += 1
                continue
            if ids not in seen:
                seen.add(ids)
                phrases.append(ids)
                texts.append("".join(chars))
                wts.append(0.0 if weights is None else float(weights[i]))
        self = cls.from_phrases(phrases, wts, texts, loop)
        self.skipped = skipped
        return self

    @classmethod
    def token_loop(cls, vocab_size: int) -> "DecodingGraph":
        """One node and a self-loop per token 1 .. V-1: unconstrained best-path decoding."""
        return cls(1, [(0, 0, v, 0.0) for v in range(1, int(vocab_size))], {0: 0.0})

    # ---- tables -----------------------------------------------------------------------------------------------------
    def host_tables(self):
        """The arrays device_tables copies, as numpy: (in_ptr, src, dst, label, col, w, final, cols)."""
        return (self.in_ptr.copy(), self.src.copy(), self.dst.copy(), self.label.copy(), self.col.copy(), self.w.copy(),
                self.final.copy(), self.cols.copy())

    def device_tables(self, device):
        """host_tables() on `device`; made once per device and kept."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError(f"DecodingGraph: device tables live on a GPU (got {device})")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(device)
        if t is None:
            t = tuple(torch.from_numpy(a).to(device) for a in self.host_tables())
            self._device[device] = t
        return t

    def accepts(self, frames: Sequence[int]) -> bool:
        """Does the graph accept the frame labelling `frames` (0 = blank) under the CTC topology?  A set simulation over the
        node and arc states of oe_ctc_graph, weights ignored."""
        nodes, arcs = {0}, set()
        for c in frames:
            c = int(c)
            if c == 0:
                nodes = nodes | {int(self.dst[a]) for a in arcs}
                arcs = set()
            else:
                nxt = set()
                for a in range(self.num_arcs):
                    if int(self.label[a]) != c:
                        continue
                    s = int(self.src[a])
                    if a in arcs or s in nodes or any(int(self.dst[x]) == s and int(self.label[x]) != c for x in arcs):
                        nxt.add(a)
                nodes, arcs = set(), nxt
        return any(self.final[q] > NEG_INF for q in nodes) or any(self.final[int(self.dst[a])] > NEG_INF for a in arcs)


@dataclass
class GraphResult:
    """One utterance decoded through a DecodingGraph.  tokens: the path collapsed (a label per arc traversal);  traversals:
    per traversal {"arc", "token", "start_frame", "end_frame" (inclusive encoder frames), "logp", "confidence" =
    exp(logp / frames)};  outputs: the traversals of arcs that carry an output, each {"output", "start_frame", "end_frame",
    "confidence"} - the span from the end of the previous output to this arc's last frame, the confidence over the traversals in
    it - and with times "start_s" / "end_s";  score: the path's value, weights and final weight included (-inf if infeasible);
    truncated: more traversals than were asked for, only the first are listed."""
    feasible: bool
    score: float
    tokens: List[int] = field(default_factory=list)
    traversals: List[dict] = field(default_factory=list)
    outputs: List[dict] = field(default_factory=list)
    truncated: bool = False

    @property
    def confidences(self) -> List[float]:
        return [t["confidence"] for t in self.traversals]


def graph_results(graph: DecodingGraph, score, n_trav, trav_arc, trav_start, trav_end, trav_logp, times=None) -> List[GraphResult]:
    """The outputs of ops.ctc_graph_decode, already on the host as nested lists (score, n_trav (B); trav_* (B, max_trav)) ->
    a GraphResult per utterance.  times: a function (start_frame, end_frame) -> (start_s, end_s) that adds "start_s" / "end_s"
    to the traversals and the outputs."""
    results = []
    for b, sc in enumerate(score):
        sc = float(sc)
        if sc == NEG_INF:
            results.append(GraphResult(False, NEG_INF))
            continue
        stored = len(trav_arc[b])
        n = min(int(n_trav[b]), stored)
        res = GraphResult(True, sc, truncated=int(n_trav[b]) > stored)
        first, logp, frames = None, 0.0, 0
        for i in range(n):
            a, s, e, lg = int(trav_arc[b][i]), int(trav_start[b][i]), int(trav_end[b][i]), float(trav_logp[b][i])
            tr = {"arc": a, "token": int(graph.label[a]), "start_frame": s, "end_frame": e, "logp": lg,
                  "confidence": math.exp(lg / (e - s + 1))}
            if times is not None:
                tr["start_s"], tr["end_s"] = times(s, e)
            res.tokens.append(tr["token"])
            res.traversals.append(tr)
            first = s if first is None else first
            logp, frames = logp + lg, frames + (e - s + 1)
            if graph.outputs[a] is not None:
                out = {"output": graph.outputs[a], "start_frame": first, "end_frame": e, "confidence": math.exp(logp / frames)}
                if times is not None:
                    out["start_s"], out["end_s"] = times(first, e)
                res.outputs.append(out)
                first, logp, frames = None, 0.0, 0
        results.append(res)
    return results
