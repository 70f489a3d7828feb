"""Loop-level numpy restatement of the grammar-constrained CTC decode that oe_ctc_graph computes (the semantics are written
out in include/openeat_hip.h), in the dtype it is given.  Written naively: every arc maximises directly over all the arcs
into its source node, so the kernel's two-best shortcut is checked independently.  A helper for the graph tests, not
collected itself."""
import itertools

import numpy as np

STAY, FROM_NODE = -1, -2


def decode(lp, Tb, num_nodes, src, dst, label, w, final, dtype=np.float64, max_trav=None):
    """lp (T, V) log-probabilities (rows t >= Tb are not read), the graph's arcs in stored order (sorted by dst) ->
    dict(score, frames (T), arcs (T), path_logp (T), n_trav, trav_arc / trav_start / trav_end / trav_logp (max_trav),
    n_state / r_state = the last frame's values).  Every sum is taken in `dtype`, in the order the header states."""
    lp = np.asarray(lp).astype(dtype)
    T, V = lp.shape
    Tb = max(min(int(Tb), T), 0)
    Q, A = int(num_nodes), len(src)
    max_trav = T if max_trav is None else int(max_trav)
    src, dst, label = (np.asarray(x, dtype=np.int64) for x in (src, dst, label))
    w, final = np.asarray(w).astype(dtype), np.asarray(final).astype(dtype)
    NEG = dtype(-np.inf)
    colv = np.clip(label, 0, V - 1)                       # a label outside [0, V): the nearest valid column
    incoming = [np.nonzero(dst == q)[0] for q in range(Q)]          # ascending arc ids
    n = np.full(Q, NEG, dtype=dtype)
    n[0] = 0
    r = np.full(A, NEG, dtype=dtype)
    bp_r = np.zeros((Tb, A), dtype=np.int64)
    bp_n = np.zeros((Tb, Q), dtype=np.int64)
    for t in range(Tb):
        nr, nn = np.full(A, NEG, dtype=dtype), np.full(Q, NEG, dtype=dtype)
        for a in range(A):
            best, mv = r[a], STAY
            s = src[a]
            if n[s] > NEG and n[s] + w[a] > best:
                best, mv = n[s] + w[a], FROM_NODE
            inc = incoming[s]
            if len(inc):
                ok = (label[inc] != label[a]) & (r[inc] > NEG)
                if ok.any():
                    cand = np.where(ok, r[inc] + w[a], NEG)
                    j = int(np.argmax(cand))              # the first maximum: the lowest arc id
                    if cand[j] > best:
                        best, mv = cand[j], int(inc[j])
            nr[a] = lp[t, colv[a]] + best
            bp_r[t, a] = mv
        for q in range(Q):
            best, mv = n[q], STAY
            inc = incoming[q]
            if len(inc):
                j = int(np.argmax(r[inc]))
                if r[inc[j]] > best:
                    best, mv = r[inc[j]], int(inc[j])
            nn[q] = lp[t, 0] + best
            bp_n[t, q] = mv
        n, r = nn, nr
    out = dict(score=NEG, frames=np.full(T, -1, dtype=np.int32), arcs=np.full(T, -1, dtype=np.int32),
               path_logp=np.zeros(T, dtype=dtype), n_trav=0, trav_arc=np.full(max_trav, -1, dtype=np.int32),
               trav_start=np.full(max_trav, -1, dtype=np.int32), trav_end=np.full(max_trav, -1, dtype=np.int32),
               trav_logp=np.zeros(max_trav, dtype=dtype), n_state=n, r_state=r)
    if Tb == 0:
        return out
    best, state = NEG, None                               # ("n", q) or ("r", a)
    for q in range(Q):
        if n[q] > NEG and final[q] > NEG and n[q] + final[q] > best:
            best, state = n[q] + final[q], ("n", q)
    for a in range(A):
        if r[a] > NEG and final[dst[a]] > NEG and r[a] + final[dst[a]] > best:
            best, state = r[a] + final[dst[a]], ("r", a)
    if state is None:
        return out
    out["score"] = best
    for t in range(Tb - 1, -1, -1):
        kind, i = state
        if kind == "r":
            out["frames"][t], out["arcs"][t], out["path_logp"][t] = label[i], i, lp[t, colv[i]]
            mv = bp_r[t, i]
            state = ("r", i) if mv == STAY else ("n", int(src[i])) if mv == FROM_NODE else ("r", int(mv))
        else:
            out["frames"][t], out["arcs"][t], out["path_logp"][t] = 0, -1, lp[t, 0]
            mv = bp_n[t, i]
            state = ("n", i) if mv == STAY else ("r", int(mv))
    assert state == ("n", 0), state
    k, t = 0, 0
    while t < Tb:
        a = out["arcs"][t]
        if a < 0:
            t += 1
            continue
        e, total = t, dtype(0)
        while e + 1 < Tb and out["arcs"][e + 1] == a:
            e += 1
        for u in range(t, e + 1):
            total = total + out["path_logp"][u]
        if k < max_trav:
            out["trav_arc"][k], out["trav_start"][k], out["trav_end"][k], out["trav_logp"][k] = a, t, e, total
        k += 1
        t = e + 1
    out["n_trav"] = k
    return out


def decode_graph(lp, Tb, g, dtype=np.float64, max_trav=None):
    """decode() on an openeat_amd.utils.decoding_graph.DecodingGraph."""
    return decode(lp, Tb, g.num_nodes, g.src, g.dst, g.label, g.w, g.final, dtype, max_trav)


def collapse(path):
    """Merge repeats, drop blanks."""
    out, prev = [], None
    for c in path:
        c = int(c)
        if c != prev and c != 0:
            out.append(c)
        prev = c
    return out


def best_weight(tokens, num_nodes, src, dst, label, w, final):
    """The best total weight (arcs + final, float64) of a graph path that spells `tokens`; -inf if there is none."""
    at = {0: 0.0}
    for tok in tokens:
        nxt = {}
        for a in range(len(src)):
            if int(label[a]) == tok and int(src[a]) in at:
                v = at[int(src[a])] + float(w[a])
                if v > nxt.get(int(dst[a]), -np.inf):
                    nxt[int(dst[a])] = v
        at = nxt
    return max((v + float(final[q]) for q, v in at.items()), default=-np.inf)


def brute_force(lp, num_nodes, src, dst, label, w, final):
    """The best score over every frame labelling of lp (T, V): its lp plus the best weight of a graph path that spells the
    labelling collapsed.  V ** T labellings."""
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    best = -np.inf
    for path in itertools.product(range(V), repeat=T):
        wt = best_weight(collapse(path), num_nodes, src, dst, label, w, final)
        if wt > -np.inf:
            best = max(best, float(sum(lp[t, c] for t, c in enumerate(path))) + wt)
    return best
