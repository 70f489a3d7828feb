"""Host side of grammar-constrained CTC decoding (ASRModel.ctc_graph_search, ops.ctc_graph_decode, ops.ctc_graph_beam_decode,
ops.ctc_graph_nbest; semantics in include/openeat_hip.h, oe_ctc_graph, oe_ctc_graph_beam and oe_ctc_graph_nbest): the token graph with the tables the kernels read, its
builders, and the records made of the kernels' outputs; GraphSet, the packed form oe_ctc_graph_logp reads; and the per-arc
label-group tables oe_ctc_graph_beam_logp reads, for a graph of either size.  No kernel here."""
import math
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

MAX_NODES = 8064                 # OE_CTC_GRAPH_MAX_NODES: 12 bytes of LDS per node
MAX_ARCS = 16384                 # OE_CTC_GRAPH_MAX_ARCS: 4 bytes of LDS per arc
BEAM_MAX_NODES = 1 << 20         # OE_CTC_GRAPH_BEAM_MAX_NODES: the state lives in global memory
BEAM_MAX_ARCS = 1 << 22          # OE_CTC_GRAPH_BEAM_MAX_ARCS
LOGP_MAX_NODES = 4096            # OE_CTC_GRAPH_LOGP_MAX_NODES: 8 bytes of LDS per node
LOGP_MAX_ARCS = 5120             # OE_CTC_GRAPH_LOGP_MAX_ARCS: 24 bytes of LDS per arc
NEG_INF = float("-inf")


class DecodingGraph:
    """DecodingGraph(num_nodes, arcs, finals, outputs=None, large=False): an epsilon-free weighted token graph.  Node 0 is the start.
    arcs = (src, dst, label, weight) each, label a token id >= 1 (blank, 0, is never a label), weight a finite natural log;
    finals = {node: weight} or one weight per node with -inf for "not final"; outputs = per arc, in the caller's order, what a
    traversal of the arc emits (a word, a phrase index, anything) or None.  The graph may be non-deterministic and may have
    self-loops, parallel arcs and unreachable nodes.

    Arcs are kept sorted by dst, stable: within a node the caller's order stays, and an arc's id is its position in that order
    (`order[id]` = the caller's index, `arc_id[caller's index]` = id).  Host tables (oe_decoding_graph): in_ptr (Q+1) int32, the
    arcs into q are in_ptr[q] .. in_ptr[q+1]-1; src, dst, label (A) int32; cols (U) int32 = the distinct labels, ascending;
    col (A) int32 = the index of label into cols; w (A) float32; final (Q) float32; and the out-adjacency oe_beam_graph adds:
    out_ptr (Q+1) int32, out_arc (A) int32 = the arc ids ordered by (src, id), the arcs leaving q are
    out_arc[out_ptr[q] .. out_ptr[q+1]-1].
    large=False: the limits are oe_ctc_graph's (8064 nodes, 16384 arcs: the dense kernel keeps the state in LDS);
    large=True: those of oe_ctc_graph_beam (2^20 nodes, 2^22 arcs), the only decoder such a graph has."""

    def __init__(self, num_nodes: int, arcs: Sequence[Sequence], finals, outputs: Optional[Sequence] = None, large: bool = False):
        Q = int(num_nodes)
        max_nodes, max_arcs = self._limits(large)
        if not 1 <= Q <= max_nodes:
            raise ValueError(f"DecodingGraph: {Q} nodes outside 1 .. {max_nodes}")
        arcs = [tuple(a) for a in arcs]
        A = len(arcs)
        if A > max_arcs:
            raise ValueError(f"DecodingGraph: {A} arcs exceed {max_arcs}")
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
        self._tables(Q, np.asarray([int(a[0]) for a in arcs], dtype=np.int32).reshape(A), np.asarray([int(a[1]) for a in arcs], dtype=np.int32).reshape(A),
                     np.asarray([int(a[2]) for a in arcs], dtype=np.int32).reshape(A), np.asarray([float(a[3]) for a in arcs], dtype=np.float32).reshape(A),
                     fin, outputs, large)

    @staticmethod
    def _limits(large: bool):
        return (BEAM_MAX_NODES, BEAM_MAX_ARCS) if large else (MAX_NODES, MAX_ARCS)

    def _tables(self, Q, src, dst, label, w, fin, outputs, large):
        """The stored form of checked arcs given in the caller's order: sorted by dst, stable, with every table."""
        A = len(src)
        self.num_nodes, self.num_arcs, self.large = Q, A, bool(large)
        self.order = np.argsort(dst, kind="stable").astype(np.int32)
        self.arc_id = np.empty(A, dtype=np.int32)
        self.arc_id[self.order] = np.arange(A, dtype=np.int32)
        self.src, self.dst, self.label, self.w = src[self.order], dst[self.order], label[self.order], w[self.order]
        self.final = fin
        self.outputs = [None] * A if outputs is None else [outputs[i] for i in self.order.tolist()]
        self.in_ptr = np.zeros(Q + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.dst, minlength=Q), out=self.in_ptr[1:])
        self.out_arc = np.argsort(self.src, kind="stable").astype(np.int32)
        self.out_ptr = np.zeros(Q + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.src, minlength=Q), out=self.out_ptr[1:])
        self.cols = np.unique(self.label).astype(np.int32)
        self.col = np.searchsorted(self.cols, self.label).astype(np.int32)
        self.skipped = 0
        self._device: Dict[object, tuple] = {}
        self._device_out: Dict[object, tuple] = {}
        self._groups: Optional[tuple] = None
        self._device_groups: Dict[object, tuple] = {}

    @classmethod
    def from_arrays(cls, num_nodes: int, src, dst, label, w, final, outputs: Optional[Sequence] = None, large: bool = False) -> "DecodingGraph":
        """DecodingGraph(num_nodes, zip(src, dst, label, w), final, outputs, large) from arrays, checked and built with numpy -
        no Python loop over the arcs, so that a graph of millions of arcs builds in seconds.  final: one weight per node,
        -inf for "not final"."""
        Q = int(num_nodes)
        max_nodes, max_arcs = cls._limits(large)
        if not 1 <= Q <= max_nodes:
            raise ValueError(f"DecodingGraph: {Q} nodes outside 1 .. {max_nodes}")
        given = [np.asarray(x) for x in (src, dst, label, w)]
        A = len(given[0])
        if any(x.shape != (A,) for x in given):
            raise ValueError(f"DecodingGraph.from_arrays: src, dst, label and w are one-dimensional and of one length, got {[x.shape for x in given]}")
        if A > max_arcs:
            raise ValueError(f"DecodingGraph: {A} arcs exceed {max_arcs}")
        if any(x.dtype.kind not in "iu" for x in given[:3]):
            raise ValueError("DecodingGraph.from_arrays: src, dst and label are integers")
        src, dst, label = (x.astype(np.int64) for x in given[:3])
        w64 = given[3].astype(np.float64)
        if A and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= Q):
            raise ValueError(f"DecodingGraph: an arc leaves the nodes 0 .. {Q - 1}")
        if A and (label.min() < 1 or label.max() > np.iinfo(np.int32).max):
            raise ValueError("DecodingGraph: a label is a token id >= 1 (0 is the blank; there are no epsilon arcs)")
        if not np.isfinite(w64).all():
            raise ValueError("DecodingGraph: a weight is finite")
        fin = np.asarray(final, dtype=np.float32)
        if fin.shape != (Q,):
            raise ValueError(f"DecodingGraph: finals is one weight per node ({Q}), got {fin.shape}")
        if np.isnan(fin).any() or np.isposinf(fin).any():
            raise ValueError("DecodingGraph: a final weight is finite, or -inf for a node that is not final")
        if outputs is not None and len(outputs) != A:
            raise ValueError(f"DecodingGraph: one output per arc ({A}), got {len(outputs)}")
        self = cls.__new__(cls)
        self._tables(Q, src.astype(np.int32), dst.astype(np.int32), label.astype(np.int32), w64.astype(np.float32), fin, outputs, large)
        return self

    # ---- builders ---------------------------------------------------------------------------------------------------
    @classmethod
    def linear(cls, tokens: Sequence[int]) -> "DecodingGraph":
        """The chain that accepts `tokens` alone, weights 0: oe_ctc_align's problem, ties included."""
        toks = [int(t) for t in tokens]
        return cls(len(toks) + 1, [(i, i + 1, t, 0.0) for i, t in enumerate(toks)], {len(toks): 0.0})

    @classmethod
    def from_phrases(cls, phrases: Sequence[Sequence[int]], weights: Optional[Sequence[float]] = None,
                     outputs: Optional[Sequence] = None, loop: bool = False, large: bool = False) -> "DecodingGraph":
        """A prefix trie over the phrases (token-id sequences of at least one label, no two alike).  All but a phrase's last
        token share the trie's arcs; its last arc is its own - it carries weights[i] (default 0) and outputs[i] (default i)
        and ends in a final node of its own, so a phrase that is the beginning of another emits only its own output.
        loop=True: the last arc returns to node 0, which is final, so sequences of phrases decode without epsilons (with
        weights, a lexicon loop with a unigram weight per word).  large: as in the constructor."""
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
        return cls(n, arcs, finals, arc_out, large)

    @classmethod
    def from_text(cls, lines: Iterable[str], token2id, weights: Optional[Sequence[float]] = None, loop: bool = False,
                  large: bool = False) -> "DecodingGraph":
        """One phrase per line, split into the recipe's character tokens (every non-space character, as
        KeywordList.from_text); a phrase's output is its text.  A line with a character token2id does not list (or maps to the
        blank) is skipped and counted in `.skipped`; empty lines and repeated phrases (the first is kept) are dropped.
        weights: one per line of `lines`.  large: as in the constructor."""
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
        self = cls.from_phrases(phrases, wts, texts, loop, large)
        self.skipped = skipped
        return self

    @classmethod
    def token_loop(cls, vocab_size: int) -> "DecodingGraph":
        """One node and a self-loop per token 1 .. V-1: unconstrained best-path decoding."""
        return cls(1, [(0, 0, v, 0.0) for v in range(1, int(vocab_size))], {0: 0.0})

    @classmethod
    def from_alternatives(cls, segments: Sequence[Sequence[Sequence[int]]], weights: Optional[Sequence[Sequence[float]]] = None) -> "DecodingGraph":
        """A transcript with alternatives (oe_ctc_graph_logp's training graph): `segments` is a sequence of segments, each a
        list of alternative token sequences ("2" / "two", several pronunciations); an empty alternative makes the segment
        optional (a filler).  weights[i][j] (default 0) is the weight of alternative j of segment i; a path's weight is the sum
        over the alternatives it takes.  The sausage is made epsilon-free by classical epsilon removal, from the end so that
        chains of optional segments work: the arcs leaving the far node of an optional segment are copied to its near node
        with the skip's weight added, and finality is carried back.  Raises if the whole transcript can be empty, if a
        segment lists an alternative twice, and if the result exceeds oe_ctc_graph_logp's limits."""
        segs = [[tuple(int(t) for t in alt) for alt in seg] for seg in segments]
        if not segs or any(len(seg) == 0 for seg in segs):
            raise ValueError("DecodingGraph.from_alternatives: at least one segment, each of at least one alternative")
        wts = [[0.0] * len(seg) for seg in segs] if weights is None else [[float(x) for x in ws] for ws in weights]
        if len(wts) != len(segs) or any(len(ws) != len(seg) for ws, seg in zip(wts, segs)):
            raise ValueError("DecodingGraph.from_alternatives: one weight per alternative of every segment")
        S = len(segs)
        n = S + 1                                                       # nodes 0 .. S are the sausage's joints
        out: List[List[tuple]] = [[] for _ in range(S + 1)]             # arcs leaving each joint, (dst, label, weight)
        inner = []                                                      # arcs inside an alternative's chain
        skip = [None] * S
        for i, (seg, ws) in enumerate(zip(segs, wts)):
            if len(set(seg)) != len(seg):
                raise ValueError(f"DecodingGraph.from_alternatives: segment {i} lists an alternative twice")
            for alt, wt in zip(seg, ws):
                if not alt:
                    skip[i] = wt
                    continue
                q = i
                for j, t in enumerate(alt):
                    nxt = i + 1 if j == len(alt) - 1 else n
                    if nxt == n:
                        n += 1
                    if q == i:
                        out[i].append((nxt, t, wt))
                    else:
                        inner.append((q, nxt, t, 0.0))
                    q = nxt
        final = {S: 0.0}
        for i in range(S - 1, -1, -1):
            if skip[i] is None:
                continue
            out[i].extend((d, t, wt + skip[i]) for d, t, wt in out[i + 1])
            if i + 1 in final:
                final[i] = final[i + 1] + skip[i]
        if 0 in final:
            raise ValueError("DecodingGraph.from_alternatives: the whole transcript can be empty")
        arcs = [(i, d, t, wt) for i in range(S + 1) for d, t, wt in out[i]] + inner
        if n > LOGP_MAX_NODES or len(arcs) > LOGP_MAX_ARCS:
            raise ValueError(f"DecodingGraph.from_alternatives: {n} nodes / {len(arcs)} arcs exceed {LOGP_MAX_NODES} / {LOGP_MAX_ARCS}")
        return cls(n, arcs, final)

    # ---- tables -----------------------------------------------------------------------------------------------------
    def host_tables(self):
        """The arrays device_tables copies, as numpy: (in_ptr, src, dst, label, col, w, final, cols)."""
        return (self.in_ptr.copy(), self.src.copy(), self.dst.copy(), self.label.copy(), self.col.copy(), self.w.copy(),
                self.final.copy(), self.cols.copy())

    def host_out_tables(self):
        """The out-adjacency oe_beam_graph adds to host_tables(), as numpy: (out_ptr, out_arc)."""
        return self.out_ptr.copy(), self.out_arc.copy()

    def _on_device(self, cache, tables, device):
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError(f"DecodingGraph: device tables live on a GPU (got {device})")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = cache.get(device)
        if t is None:
            t = tuple(torch.from_numpy(a).to(device) for a in tables())
            cache[device] = t
        return t

    def device_tables(self, device):
        """host_tables() on `device`; made once per device and kept."""
        return self._on_device(self._device, self.host_tables, device)

    def device_out_tables(self, device):
        """host_out_tables() on `device`; made once per device and kept."""
        return self._on_device(self._device_out, self.host_out_tables, device)

    def host_group_tables(self):
        """The label-group tables oe_beam_logp_graph adds to host_tables() and host_out_tables(), as numpy, made once and kept:
        (in_grp, in_xg, out_grp, out_xg, inv).  The groups and their ids are _group_tables' (those of a GraphSet of this one
        graph): in_grp[a] = the in-group of dst[a] that holds a, out_grp[a] = the out-group of src[a] that holds a; in_xg,
        out_xg and inv as in oe_graph_set."""
        if self._groups is None:
            Q, A, U = self.num_nodes, self.num_arcs, len(self.cols)

            def group_of(perm, gstart):
                grp = np.empty(A, dtype=np.int32)
                grp[perm] = np.searchsorted(gstart[:int(np.count_nonzero(gstart < A))], np.arange(A), side="right") - 1
                return grp

            in_perm, in_gstart, _, in_xg = _group_tables(self.dst, self.src, self.col, Q, U)
            out_perm, out_gstart, _, out_xg = _group_tables(self.src, self.dst, self.col, Q, U)
            inv = np.full((int(self.cols.max()) if U else 0) + 1, -1, dtype=np.int32)
            inv[0] = 0
            inv[self.cols] = 1 + np.arange(U, dtype=np.int32)
            self._groups = (group_of(in_perm, in_gstart), in_xg, group_of(out_perm, out_gstart), out_xg, inv)
        return tuple(a.copy() for a in self._groups)

    def device_group_tables(self, device):
        """host_group_tables() on `device`; made once per device and kept."""
        return self._on_device(self._device_groups, self.host_group_tables, device)

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


def _group_tables(node, other, col, Q, U):
    """The label groups of the arcs at their `node` end (dst: in-groups, src: out-groups): perm (A) = the arcs ordered by
    (node, col, id); a group is a maximal run of one (node, col); gstart (A+1) = the groups' first positions in perm, padded
    with A; gptr (Q+1) = the first group of each node; xg (A) = the group of node other[a] that carries col[a], or -1."""
    A = len(node)
    perm = np.lexsort((np.arange(A), col, node)).astype(np.int32)
    key = node[perm].astype(np.int64) * (U + 1) + col[perm]
    starts = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if A else np.zeros(0, dtype=np.int64)
    gstart = np.full(A + 1, A, dtype=np.int32)
    gstart[:len(starts)] = starts
    gkey = key[starts]
    gptr = np.searchsorted(gkey, np.arange(Q + 1, dtype=np.int64) * (U + 1), side="left").astype(np.int32)
    want = other.astype(np.int64) * (U + 1) + col
    pos = np.searchsorted(gkey, want)
    hit = (pos < len(gkey)) & (gkey[np.minimum(pos, max(len(gkey) - 1, 0))] == want) if len(gkey) else np.zeros(A, dtype=bool)
    xg = np.where(hit, pos, -1).astype(np.int32)
    return perm, gstart, gptr, xg


class GraphSet:
    """GraphSet(graphs): G DecodingGraphs packed for oe_ctc_graph_logp (oe_graph_set in include/openeat_hip.h).  One `cols`,
    the union of the graphs' labels, so one compact lp row serves every utterance; node_off / arc_off (G+1) the graphs'
    ranges in the concatenated tables; every index in a table is local to its graph.  tables: name -> numpy array, the fields
    of oe_graph_set; `graph_tables(i)` gives graph i's slices."""
    MAX_NODES, MAX_ARCS = LOGP_MAX_NODES, LOGP_MAX_ARCS
    PER_NODE = ("final",)                                               # n entries per graph
    PER_NODE1 = ("in_ptr", "in_gptr", "out_gptr")                       # n + 1
    PER_ARC = ("src", "dst", "label", "col", "w", "in_perm", "in_xg", "out_perm", "out_xg", "col_perm")
    PER_ARC1 = ("in_gstart", "out_gstart")
    NAMES = ("node_off", "arc_off", "in_ptr", "src", "dst", "label", "col", "w", "final", "cols", "in_gptr", "in_gstart", "in_perm",
             "in_xg", "out_gptr", "out_gstart", "out_perm", "out_xg", "col_ptr", "col_perm", "inv")

    def __init__(self, graphs: Sequence[DecodingGraph]):
        graphs = [graphs] if isinstance(graphs, DecodingGraph) else list(graphs)
        if not graphs or not all(isinstance(g, DecodingGraph) for g in graphs):
            raise TypeError("GraphSet: one or more DecodingGraphs")
        for i, g in enumerate(graphs):
            if g.num_nodes > LOGP_MAX_NODES or not 1 <= g.num_arcs <= LOGP_MAX_ARCS:
                raise ValueError(f"GraphSet: graph {i} has {g.num_nodes} nodes / {g.num_arcs} arcs; the limits are {LOGP_MAX_NODES} "
                                 f"nodes and 1 .. {LOGP_MAX_ARCS} arcs")
        self.graphs = graphs
        self.cols = np.unique(np.concatenate([g.label for g in graphs])).astype(np.int32)
        U = len(self.cols)
        parts = {k: [] for k in self.NAMES}
        for g in graphs:
            Q, A = g.num_nodes, g.num_arcs
            col = np.searchsorted(self.cols, g.label).astype(np.int32)
            in_perm, in_gstart, in_gptr, in_xg = _group_tables(g.dst, g.src, col, Q, U)
            out_perm, out_gstart, out_gptr, out_xg = _group_tables(g.src, g.dst, col, Q, U)
            col_perm = np.lexsort((np.arange(A), col)).astype(np.int32)
            col_ptr = np.searchsorted(col[col_perm], np.arange(U + 1)).astype(np.int32)
            for k, v in (("in_ptr", g.in_ptr), ("src", g.src), ("dst", g.dst), ("label", g.label), ("col", col), ("w", g.w),
                         ("final", g.final), ("in_gptr", in_gptr), ("in_gstart", in_gstart), ("in_perm", in_perm), ("in_xg", in_xg),
                         ("out_gptr", out_gptr), ("out_gstart", out_gstart), ("out_perm", out_perm), ("out_xg", out_xg),
                         ("col_ptr", col_ptr), ("col_perm", col_perm)):
                parts[k].append(v)
        self.num_graphs = len(graphs)
        self.node_off = np.concatenate(([0], np.cumsum([g.num_nodes for g in graphs]))).astype(np.int32)
        self.arc_off = np.concatenate(([0], np.cumsum([g.num_arcs for g in graphs]))).astype(np.int32)
        self.Qmax = max(g.num_nodes for g in graphs)
        self.Amax = max(g.num_arcs for g in graphs)
        inv = np.full(int(self.cols.max()) + 1, -1, dtype=np.int32)
        inv[0] = 0
        inv[self.cols] = 1 + np.arange(U, dtype=np.int32)
        self.tables = {k: np.concatenate(v) for k, v in parts.items() if v}
        self.tables.update(node_off=self.node_off, arc_off=self.arc_off, cols=self.cols, inv=inv)
        self._device: Dict[object, dict] = {}

    def graph_tables(self, i: int) -> dict:
        """Graph i's slices of the concatenated tables (col and col_ptr refer to the set's cols)."""
        q0, q1, a0, a1 = int(self.node_off[i]), int(self.node_off[i + 1]), int(self.arc_off[i]), int(self.arc_off[i + 1])
        U = len(self.cols)
        t = {k: self.tables[k][q0:q1] for k in self.PER_NODE}
        t.update({k: self.tables[k][q0 + i:q1 + i + 1] for k in self.PER_NODE1})
        t.update({k: self.tables[k][a0:a1] for k in self.PER_ARC})
        t.update({k: self.tables[k][a0 + i:a1 + i + 1] for k in self.PER_ARC1})
        t["col_ptr"] = self.tables["col_ptr"][i * (U + 1):(i + 1) * (U + 1)]
        return t

    def device_tables(self, device) -> dict:
        """tables on `device`; made once per device and kept."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError(f"GraphSet: device tables live on a GPU (got {device})")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(device)
        if t is None:
            t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in self.tables.items()}
            self._device[device] = t
        return t


@dataclass
class GraphResult:
    """One utterance decoded through a DecodingGraph.  tokens: the path collapsed (a label per arc traversal);  traversals:
    per traversal {"arc", "token", "start_frame", "end_frame" (inclusive encoder frames), "logp", "confidence" =
    exp(logp / frames)};  outputs: the traversals of arcs that carry an output, each {"output", "start_frame", "end_frame",
    "confidence"} - the span from the end of the previous output to this arc's last frame, the confidence over the traversals in
    it - and with times "start_s" / "end_s";  score: the path's value, weights and final weight included (-inf if infeasible);
    truncated: more traversals than were asked for, only the first are listed;  log_mass, posterior (ctc_graph_search with
    posterior=True, else None): the graph's total log-likelihood on the normalised posteriors (oe_ctc_graph_logp) - with zero
    weights log P(the labelling is in the grammar) - and exp(score - log_mass), the best path's share of it (with
    posterior_beam: of the beam-pruned sum, oe_ctc_graph_beam_logp);  nbest
    (ctc_graph_search with nbest=K, else None): the K best distinct paths as GraphHypothesis, best first."""
    feasible: bool
    score: float
    tokens: List[int] = field(default_factory=list)
    traversals: List[dict] = field(default_factory=list)
    outputs: List[dict] = field(default_factory=list)
    truncated: bool = False
    log_mass: Optional[float] = None
    posterior: Optional[float] = None
    nbest: Optional[List["GraphHypothesis"]] = None

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


@dataclass
class GraphHypothesis:
    """One of the n best paths of an utterance through a DecodingGraph (oe_ctc_graph_nbest).  tokens: a label per arc of the
    path;  arcs: the arc ids;  outputs: the outputs of the arcs that carry one, in path order;  score: the value of the path's
    best alignment, weights and final weight included (after graph_attention_rescoring: the mixed score);  rank: the position
    in the first pass's list, 0 the best (-1 with score -inf: the infeasible result of graph_attention_rescoring);  truncated: the path has more arcs than were asked for, only the first are listed."""
    tokens: List[int] = field(default_factory=list)
    arcs: List[int] = field(default_factory=list)
    outputs: List = field(default_factory=list)
    score: float = NEG_INF
    rank: int = 0
    truncated: bool = False

    @property
    def feasible(self) -> bool:
        return self.score > NEG_INF


def graph_hypotheses(graph: DecodingGraph, n_hyp, hyp_score, hyp_len, hyp_arcs, hyp_tokens) -> List[List[GraphHypothesis]]:
    """The outputs of ops.ctc_graph_nbest, already on the host as nested lists (n_hyp (B); hyp_score, hyp_len (B, K); hyp_arcs,
    hyp_tokens (B, K, max_len)) -> per utterance the list of its GraphHypothesis, best first (empty if infeasible)."""
    results = []
    for b, n in enumerate(n_hyp):
        hyps = []
        for k in range(int(n)):
            stored = len(hyp_arcs[b][k])
            m = min(int(hyp_len[b][k]), stored)
            arcs = [int(a) for a in hyp_arcs[b][k][:m]]
            hyps.append(GraphHypothesis([int(t) for t in hyp_tokens[b][k][:m]], arcs, [graph.outputs[a] for a in arcs if graph.outputs[a] is not None],
                                        float(hyp_score[b][k]), k, int(hyp_len[b][k]) > stored))
        results.append(hyps)
    return results
