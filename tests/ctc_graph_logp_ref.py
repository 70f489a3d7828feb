"""A float64 numpy restatement of oe_ctc_graph_logp (include/openeat_hip.h): the graph CTC likelihood, alpha, beta, the
occupancies and the gradient with respect to raw logits, written naively - "every incoming arc of another label" is a direct
sum over those arcs (a list of (arc, other arc) pairs), never a subtraction and never a prefix / suffix sweep - and an
enumerator: every labelling of the frames x the log-sum of the weights of every graph path that spells its collapse.
A helper; the tests do not collect it."""
import itertools

import numpy as np

NEG = -np.inf


def seg_lse(vals, ids, n):
    """out[i] = log sum exp of vals[ids == i] (-inf for an empty or all -inf segment)."""
    vals = np.asarray(vals, dtype=np.float64)
    m = np.full(n, NEG)
    np.maximum.at(m, ids, vals)
    safe = np.where(np.isfinite(m), m, 0.0)
    s = np.zeros(n)
    with np.errstate(over="ignore", invalid="ignore"):
        np.add.at(s, ids, np.exp(vals - safe[ids]))
    with np.errstate(divide="ignore"):
        return np.where(s > 0, safe + np.log(s), NEG)


def lse(vals):
    vals = np.asarray(vals, dtype=np.float64).ravel()
    return float(seg_lse(vals, np.zeros(len(vals), dtype=np.int64), 1)[0]) if len(vals) else NEG


def other_label_pairs(src, dst, label, Q):
    """(a, a') for every a' with dst[a'] == src[a] and label[a'] != label[a]."""
    A = len(src)
    into = [[] for _ in range(Q)]
    for a in range(A):
        into[int(dst[a])].append(a)
    first, second = [], []
    for a in range(A):
        for x in into[int(src[a])]:
            if label[x] != label[a]:
                first.append(a)
                second.append(x)
    return np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def graph_logp(lp, graph):
    """lp (Tb, V) float64 log-probabilities (any values: they need not be normalised), graph a DecodingGraph ->
    dict(logz, alpha_n (Tb, Q), alpha_r (Tb, A), beta_n, beta_r, occ (Tb, V)); logz -inf and occ zeros if infeasible."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, V = lp.shape
    Q, A = graph.num_nodes, graph.num_arcs
    src, dst, label = graph.src.astype(np.int64), graph.dst.astype(np.int64), graph.label.astype(np.int64)
    w, fin = graph.w.astype(np.float64), graph.final.astype(np.float64)
    pa, pb = other_label_pairs(src, dst, label, Q)
    ar = np.arange(A)
    an, arr = np.full((Tb, Q), NEG), np.full((Tb, A), NEG)
    n, r = np.full(Q, NEG), np.full(A, NEG)
    n[0] = 0.0
    for t in range(Tb):
        cand = seg_lse(np.concatenate([r, n[src] + w, r[pb] + w[pa]]), np.concatenate([ar, ar, pa]), A)
        nn = lp[t, 0] + seg_lse(np.concatenate([n, r]), np.concatenate([np.arange(Q), dst]), Q)
        r = lp[t, label] + cand
        n = nn
        an[t], arr[t] = n, r
    out = dict(logz=NEG, alpha_n=an, alpha_r=arr, beta_n=np.full((Tb, Q), NEG), beta_r=np.full((Tb, A), NEG), occ=np.zeros((Tb, V)))
    if Tb == 0:
        return out
    logz = lse(np.concatenate([n + fin, r + fin[dst]]))
    out["logz"] = logz
    if not np.isfinite(logz):
        return out
    bn, br = fin.copy(), fin[dst].copy()
    for t in range(Tb - 1, -1, -1):
        if t < Tb - 1:
            y = w + lp[t + 1, label] + br                               # enter arc a'' at frame t + 1
            nbr = seg_lse(np.concatenate([lp[t + 1, label] + br, lp[t + 1, 0] + bn[dst], y[pa]]), np.concatenate([ar, ar, pb]), A)
            bn = seg_lse(np.concatenate([lp[t + 1, 0] + bn, y]), np.concatenate([np.arange(Q), src]), Q)
            br = nbr
        out["beta_n"][t], out["beta_r"][t] = bn, br
        with np.errstate(invalid="ignore"):
            on, orr = np.exp(an[t] + bn - logz), np.exp(arr[t] + br - logz)
        out["occ"][t, 0] = np.nansum(on)
        np.add.at(out["occ"][t], label, np.nan_to_num(orr))
    return out


def logp_and_grad(logits, hlens, graphs, graph_of=None, g=None, normalized=False):
    """logits (B, T, V), hlens (B), graphs a list of DecodingGraphs (or one), graph_of (B) or None -> logp (B) float64 (-inf:
    infeasible), dlogits (B, T, V) float64 = d sum_b g[b] logp[b] / d logits for raw logits (zeros where infeasible, t >= Tb)."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, V = logits.shape
    graphs = graphs if isinstance(graphs, (list, tuple)) else [graphs]
    graph_of = [0] * B if graph_of is None else graph_of
    g = np.ones(B) if g is None else g
    logp, grad = np.full(B, NEG), np.zeros_like(logits)
    for b in range(B):
        Tb = int(min(max(hlens[b], 0), T))
        lp = logits[b, :Tb] if normalized else log_softmax(logits[b, :Tb])
        res = graph_logp(lp, graphs[int(graph_of[b])])
        logp[b] = res["logz"]
        if np.isfinite(res["logz"]) and not normalized:
            grad[b, :Tb] = g[b] * (res["occ"] - np.exp(lp))
    return logp, grad


def random_graph(rng, Q, A, V, final_p=0.4):
    """Non-deterministic, with self-loops, parallel arcs (same and different labels), unreachable nodes and dead ends."""
    arcs = []
    for _ in range(A):
        s, d = int(rng.integers(0, Q)), int(rng.integers(0, Q))
        arcs.append((s, d, int(rng.integers(1, V)), float(rng.normal() * 0.7)))
    if A >= 2:
        arcs[1] = (arcs[0][0], arcs[0][1], arcs[0][2], 0.3)              # a parallel arc of the same label
    finals = {q: float(rng.normal() * 0.5) for q in range(Q) if rng.random() < final_p}
    if not finals:
        finals = {int(rng.integers(0, Q)): 0.0}
    from openeat_amd.utils.decoding_graph import DecodingGraph
    return DecodingGraph(Q, arcs, finals)


def collapse(frames):
    out, prev = [], 0
    for c in frames:
        if c != 0 and c != prev:
            out.append(int(c))
        prev = c
    return out


def path_weight(graph, tokens):
    """log of the sum over the graph's paths that spell `tokens` of exp(arc weights + final weight)."""
    f = np.full(graph.num_nodes, NEG)
    f[0] = 0.0
    for tok in tokens:
        nxt = np.full(graph.num_nodes, NEG)
        for a in range(graph.num_arcs):
            if int(graph.label[a]) == tok and f[int(graph.src[a])] > NEG:
                nxt[int(graph.dst[a])] = np.logaddexp(nxt[int(graph.dst[a])], f[int(graph.src[a])] + float(graph.w[a]))
        f = nxt
    return lse(f + graph.final.astype(np.float64))


def enumerate_logz(lp, graph):
    """The definition: log of the sum over all V^Tb labellings of exp(sum_t lp[t, c_t]) * the weight of its collapse."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, V = lp.shape
    if Tb == 0:
        return NEG
    cache, terms = {}, []
    for frames in itertools.product(range(V), repeat=Tb):
        key = tuple(collapse(frames))
        if key not in cache:
            cache[key] = path_weight(graph, key)
        if cache[key] > NEG:
            terms.append(cache[key] + sum(lp[t, c] for t, c in enumerate(frames)))
    return lse(terms)
