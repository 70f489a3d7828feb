"""A float64 numpy restatement of oe_ctc_graph_beam_logp (include/openeat_hip.h): the beam-pruned graph CTC likelihood, the
occupancies of the pruned lattice and the gradient with respect to raw logits.  Two formulations:
  pruned_logp       written like ctc_graph_logp_ref.graph_logp: a naive list of (arc, other arc) pairs, a dense state, and a mask
                    (-inf) for pruning;
  pruned_logp_fast  for hub graphs, where the pair list is quadratic: per (node, label) group LSEs, and "every group of another
                    label" as a sum of the groups before and behind in the linear domain against the node's maximum - sums of
                    non-negative numbers only, never a subtraction.
A helper; the tests do not collect it."""
import numpy as np

import ctc_graph_logp_ref as R

NEG = -np.inf


def _prune(n, r, beam, stats):
    """Mask the states below best - beam in place; stats = [gap, cut]."""
    allv = np.concatenate([n, r])
    f = np.isfinite(allv)
    if f.any():
        thr = allv[f].max() - beam
        if np.isfinite(thr):
            stats[0] = min(stats[0], float(np.abs(allv[f] - thr).min()))
            stats[1] += int((allv[f] < thr).sum())
            n[n < thr] = NEG
            r[r < thr] = NEG


def _occ(an, arr, bn, br, logz, label, V):
    with np.errstate(invalid="ignore"):
        on, orr = np.exp(an + bn - logz), np.exp(arr + br - logz)
    row = np.zeros(V)
    row[0] = np.nansum(on)
    np.add.at(row, label, np.nan_to_num(orr))
    return row


def _result(logz, occ, surv, stats):
    return dict(logz=logz, occ=occ, survivors=surv, gap=stats[0], cut=stats[1])


def pruned_logp(lp, graph, beam, pairs=None):
    """lp (Tb, V) float64 log-probabilities, graph a DecodingGraph, beam >= 0 or inf -> dict(logz, occ (Tb, V), survivors (the
    per-frame survivor counts), gap (the smallest |alpha - thr_t| over all finite states and pruned frames; inf if none), cut
    (the number of states cut)); logz -inf and occ zeros if infeasible."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, V = lp.shape
    Q, A = graph.num_nodes, graph.num_arcs
    src, dst, label = graph.src.astype(np.int64), graph.dst.astype(np.int64), graph.label.astype(np.int64)
    w, fin = graph.w.astype(np.float64), graph.final.astype(np.float64)
    pa, pb = pairs if pairs is not None else R.other_label_pairs(src, dst, label, Q)
    ar, qs = np.arange(A), np.arange(Q)
    n, r = np.full(Q, NEG), np.full(A, NEG)
    n[0] = 0.0
    an, arr = np.full((Tb, Q), NEG), np.full((Tb, A), NEG)
    stats, surv = [np.inf, 0], []
    for t in range(Tb):
        cand = R.seg_lse(np.concatenate([r, n[src] + w, r[pb] + w[pa]]), np.concatenate([ar, ar, pa]), A)
        nn = lp[t, 0] + R.seg_lse(np.concatenate([n, r]), np.concatenate([qs, dst]), Q)
        r = lp[t, label] + cand
        n = nn
        if t < Tb - 1:
            _prune(n, r, beam, stats)
        an[t], arr[t] = n, r
        surv.append(int(np.isfinite(n).sum() + np.isfinite(r).sum()))
    occ = np.zeros((Tb, V))
    if Tb == 0:
        return _result(NEG, occ, surv, stats)
    logz = R.lse(np.concatenate([n + fin, r + fin[dst]]))
    if np.isfinite(logz):
        bn, br = fin.copy(), fin[dst].copy()
        for t in range(Tb - 1, -1, -1):
            if t < Tb - 1:
                y = w + lp[t + 1, label] + br
                nbr = R.seg_lse(np.concatenate([lp[t + 1, label] + br, lp[t + 1, 0] + bn[dst], y[pa]]), np.concatenate([ar, ar, pb]), A)
                bn = R.seg_lse(np.concatenate([lp[t + 1, 0] + bn, y]), np.concatenate([qs, src]), Q)
                br = nbr
            bn = np.where(np.isfinite(an[t]), bn, NEG)                     # the sub-lattice
            br = np.where(np.isfinite(arr[t]), br, NEG)
            occ[t] = _occ(an[t], arr[t], bn, br, logz, label, V)
    return _result(logz, occ, surv, stats)


class _Groups:
    """The (node, label) groups of the arcs at their `node` end; xg[a] = the group of other[a] that carries label[a], or -1."""

    def __init__(self, node, other, label, Q):
        K = int(label.max()) + 2 if len(label) else 2
        self.Q = Q
        self.keys, self.gid = np.unique(node * K + label, return_inverse=True)
        self.gnode = self.keys // K
        want = other * K + label
        pos = np.minimum(np.searchsorted(self.keys, want), len(self.keys) - 1)
        self.xg = np.where(self.keys[pos] == want, pos, -1)
        first = np.searchsorted(self.gnode, np.arange(Q + 1))
        self.multi = [(int(first[q]), int(first[q + 1])) for q in np.flatnonzero(np.diff(first) >= 2)]

    def sums(self, vals):
        """vals (A) log-domain -> (tot (Q): LSE of every arc at the node, excl (groups): LSE of the node's arcs outside the
        group).  Linear sums against the node's maximum; the exclusion adds the groups before and behind."""
        ng = len(self.keys)
        gv = R.seg_lse(vals, self.gid, ng)
        m = np.full(self.Q, NEG)
        np.maximum.at(m, self.gnode, gv)
        safe = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(gv - safe[self.gnode])
        tot = np.zeros(self.Q)
        np.add.at(tot, self.gnode, e)
        excl = np.zeros(ng)
        for lo, hi in self.multi:
            seg = e[lo:hi]
            c, cr = np.cumsum(seg), np.cumsum(seg[::-1])[::-1]
            excl[lo + 1:hi] += c[:-1]
            excl[lo:hi - 1] += cr[1:]
        with np.errstate(divide="ignore"):
            return safe + np.log(tot), safe[self.gnode] + np.log(excl)


def pruned_logp_fast(lp, graph, beam):
    """pruned_logp without the pair list: O(A) per frame on a hub graph."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, V = lp.shape
    Q, A = graph.num_nodes, graph.num_arcs
    src, dst, label = graph.src.astype(np.int64), graph.dst.astype(np.int64), graph.label.astype(np.int64)
    w, fin = graph.w.astype(np.float64), graph.final.astype(np.float64)
    gin, gout = _Groups(dst, src, label, Q), _Groups(src, dst, label, Q)

    def other(groups, vals, at):
        """per arc: LSE of vals over the arcs at node at[a] of another label than a's"""
        tot, excl = groups.sums(vals)
        return tot, np.where(groups.xg >= 0, excl[np.maximum(groups.xg, 0)], tot[at])

    n, r = np.full(Q, NEG), np.full(A, NEG)
    n[0] = 0.0
    an, arr = np.full((Tb, Q), NEG), np.full((Tb, A), NEG)
    stats, surv = [np.inf, 0], []
    for t in range(Tb):
        tot, x = other(gin, r, src)
        nn = lp[t, 0] + np.logaddexp(n, tot)
        r = lp[t, label] + np.logaddexp(r, w + np.logaddexp(n[src], x))
        n = nn
        if t < Tb - 1:
            _prune(n, r, beam, stats)
        an[t], arr[t] = n, r
        surv.append(int(np.isfinite(n).sum() + np.isfinite(r).sum()))
    occ = np.zeros((Tb, V))
    if Tb == 0:
        return _result(NEG, occ, surv, stats)
    logz = R.lse(np.concatenate([n + fin, r + fin[dst]]))
    if np.isfinite(logz):
        bn, br = fin.copy(), fin[dst].copy()
        for t in range(Tb - 1, -1, -1):
            if t < Tb - 1:
                tot, x = other(gout, w + lp[t + 1, label] + br, dst)
                br = np.logaddexp(np.logaddexp(lp[t + 1, label] + br, lp[t + 1, 0] + bn[dst]), x)
                bn = np.logaddexp(lp[t + 1, 0] + bn, tot)
            bn = np.where(np.isfinite(an[t]), bn, NEG)
            br = np.where(np.isfinite(arr[t]), br, NEG)
            occ[t] = _occ(an[t], arr[t], bn, br, logz, label, V)
    return _result(logz, occ, surv, stats)


def logp_and_grad(logits, hlens, graph, beam, g=None, fast=False):
    """logits (B, T, V) raw, hlens (B), one DecodingGraph -> logp (B) float64 (-inf: infeasible), dlogits (B, T, V) float64 =
    d sum_b g[b] logp[b] / d logits with the survivor sets held fixed, and the per-utterance result dicts."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, V = logits.shape
    g = np.ones(B) if g is None else g
    logp, grad, results = np.full(B, NEG), np.zeros_like(logits), []
    for b in range(B):
        Tb = int(min(max(hlens[b], 0), T))
        lp = R.log_softmax(logits[b, :Tb])
        res = (pruned_logp_fast if fast else pruned_logp)(lp, graph, beam)
        results.append(res)
        logp[b] = res["logz"]
        if np.isfinite(res["logz"]):
            grad[b, :Tb] = g[b] * (res["occ"] - np.exp(lp))
    return logp, grad, results
