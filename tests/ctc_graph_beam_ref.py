"""Numpy restatement of the beam-pruned graph decode that oe_ctc_graph_beam computes (the semantics are written out in
include/openeat_hip.h), in the dtype it is given, in the header's order of operations: per node the two best incoming values,
the maximum first and then + w.  Dense and vectorised over the states - no active list, no stamps, no push - so the kernel's
token passing is checked against a different formulation; 10^5 nodes at T <= 16 take seconds.  A helper for the beam tests, not
collected itself."""
import numpy as np

STAY, FROM_NODE = -1, -2
OK, INFEASIBLE, OVERFLOW = 0, 1, 2


def _best_per_node(dst, r, mask, Q):
    """Per node the best r over the arcs into it that `mask` admits, the lowest id on ties -> (value (Q), id (Q), -1: none)."""
    ids = np.nonzero(mask & (r > -np.inf))[0]
    val = np.full(Q, -np.inf, dtype=r.dtype)
    arc = np.full(Q, -1, dtype=np.int64)
    if len(ids):
        with np.errstate(invalid="ignore"):
            order = ids[np.lexsort((ids, -r[ids], dst[ids]))]       # by node, then greatest value, then lowest id
        first = np.concatenate(([True], dst[order][1:] != dst[order][:-1]))
        val[dst[order[first]]] = r[order[first]]
        arc[dst[order[first]]] = order[first]
    return val, arc


def decode(lp, Tb, num_nodes, src, dst, label, w, final, beam=np.inf, max_active=None, dtype=np.float64, max_trav=None):
    """lp (T, V) log-probabilities (rows t >= Tb are not read), the graph's arcs in stored order (sorted by dst) ->
    dict(score, frames (T), arcs (T), path_logp (T), n_trav, trav_arc / trav_start / trav_end / trav_logp (max_trav), status,
    peak, pruned = the number of states each frame's pruning removed (Tb entries, the last 0), at_thr = the number of states
    that survived a frame's pruning with a value equal to its threshold, survivors = the per-frame survivor counts,
    n_state / r_state = the last frame's values).  max_active None: Q + A."""
    lp = np.asarray(lp).astype(dtype)
    T, V = lp.shape
    Tb = max(min(int(Tb), T), 0)
    Q, A = int(num_nodes), len(src)
    max_trav = T if max_trav is None else int(max_trav)
    max_active = Q + A if max_active is None else int(max_active)
    src, dst, label = (np.asarray(x, dtype=np.int64) for x in (src, dst, label))
    w, final = np.asarray(w).astype(dtype), np.asarray(final).astype(dtype)
    beam = dtype(beam)
    NEG = dtype(-np.inf)
    colv = np.clip(label, 0, V - 1)                       # a label outside [0, V): the nearest valid column
    n = np.full(Q, NEG, dtype=dtype)
    n[0] = 0
    r = np.full(A, NEG, dtype=dtype)
    bp_r, bp_n, pruned, at_thr, survivors = [], [], [], [], []
    out = dict(score=NEG, frames=np.full(T, -1, dtype=np.int32), arcs=np.full(T, -1, dtype=np.int32),
               path_logp=np.zeros(T, dtype=dtype), n_trav=0, trav_arc=np.full(max_trav, -1, dtype=np.int32),
               trav_start=np.full(max_trav, -1, dtype=np.int32), trav_end=np.full(max_trav, -1, dtype=np.int32),
               trav_logp=np.zeros(max_trav, dtype=dtype), status=INFEASIBLE, peak=0, pruned=pruned, at_thr=at_thr, survivors=survivors,
               n_state=n, r_state=r)
    every = np.ones(A, dtype=bool)
    for t in range(Tb):
        v1, id1 = _best_per_node(dst, r, every, Q)
        c1 = np.where(id1 >= 0, label[np.maximum(id1, 0)], -1)
        v2, id2 = _best_per_node(dst, r, label != c1[dst], Q)
        f1, f2 = v1 > n, v2 > n                            # the node is kept unless the arc is strictly greater
        m1, m2 = np.where(f1, v1, n), np.where(f2, v2, n)
        other = c1[src] != label
        m = np.where(other, m1[src], m2[src])
        via = np.where(other, np.where(f1[src], id1[src], FROM_NODE), np.where(f2[src], id2[src], FROM_NODE))
        with np.errstate(invalid="ignore"):
            cand = m + w                                   # the weight is added to the maximum
            take = cand > r                                # the stay is kept unless strictly greater
            nr = lp[t, colv] + np.where(take, cand, r)
            nn = lp[t, 0] + m1
        bp_r.append(np.where(take, via, STAY))
        bp_n.append(np.where(f1, id1, STAY))
        n, r = nn.astype(dtype), nr.astype(dtype)
        cut = equal = 0
        if t < Tb - 1:
            best = max(n.max(), r.max() if A else NEG)
            with np.errstate(invalid="ignore"):
                thr = dtype(best - beam)                   # one subtraction in dtype
            kn, kr = (n > NEG) & (n < thr), (r > NEG) & (r < thr)   # a state equal to thr survives
            cut, equal = int(kn.sum() + kr.sum()), int((n == thr).sum() + (r == thr).sum()) if thr > NEG else 0
            n[kn], r[kr] = NEG, NEG
        pruned.append(cut)
        at_thr.append(equal)
        alive = int((n > NEG).sum() + (r > NEG).sum())
        survivors.append(alive)
        out["n_state"], out["r_state"] = n, r
        if alive > max_active:
            out["status"], out["peak"] = OVERFLOW, alive
            return out
        out["peak"] = max(out["peak"], alive)
    if Tb == 0:
        return out
    with np.errstate(invalid="ignore"):
        ends = np.concatenate((n + final, r + final[dst]))  # nodes by ascending q, then arcs by ascending id
    state = int(np.argmax(ends))                            # the first maximum
    if not ends[state] > NEG:
        return out
    out["score"], out["status"] = ends[state], OK
    for t in range(Tb - 1, -1, -1):
        if state >= Q:
            a = state - Q
            out["frames"][t], out["arcs"][t], out["path_logp"][t] = label[a], a, lp[t, colv[a]]
            mv = int(bp_r[t][a])
            state = state if mv == STAY else int(src[a]) if mv == FROM_NODE else Q + mv
        else:
            out["frames"][t], out["arcs"][t], out["path_logp"][t] = 0, -1, lp[t, 0]
            mv = int(bp_n[t][state])
            state = state if mv == STAY else Q + mv
    assert state == 0, state
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


def decode_graph(lp, Tb, g, beam=np.inf, max_active=None, dtype=np.float64, max_trav=None):
    """decode() on an openeat_amd.utils.decoding_graph.DecodingGraph."""
    return decode(lp, Tb, g.num_nodes, g.src, g.dst, g.label, g.w, g.final, beam, max_active, dtype, max_trav)
