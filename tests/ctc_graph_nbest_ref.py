"""Loop-level numpy restatement of the n-best grammar-constrained CTC decode that oe_ctc_graph_nbest computes (the semantics
are written out in include/openeat_hip.h), in the dtype it is given.  Written naively: every arc scans the arcs into its
source node and every selection sorts its whole candidate list, so the kernel's shortcuts (the unfiltered node list reused,
the merge of sorted lists) are checked independently.  Histories are tuples; identity="hash" makes identity the device's
64-bit hash, restated here.  Also the brute force: every arc path of at most Tb arcs, scored by ctc_graph_ref.decode on its
linear chain.  A helper for the n-best graph tests, not collected itself."""
import numpy as np

import ctc_graph_ref as R

ARCS, TOKENS = 0, 1
MASK = (1 << 64) - 1


def mix(h, ident):
    """The device's history hash: the splitmix64 finaliser over (h, id + 1); the empty history is 0."""
    z = (h + 0x9E3779B97F4A7C15 * (ident + 1)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def select_k(cands, K):
    """cands: (value, key, path) in candidate order -> the first K of the stable descending sort whose key is not taken yet."""
    order = sorted((c for c in cands if c[0] > -np.inf), key=lambda c: -float(c[0]))       # sorted() is stable
    out, taken = [], set()
    for c in order:
        if c[1] in taken:
            continue
        out.append(c)
        taken.add(c[1])
        if len(out) == K:
            break
    return out


def nbest(lp, Tb, num_nodes, src, dst, label, col, w, final, K, distinct=ARCS, dtype=np.float32, identity="tuple", max_len=None,
          keys_seen=None):
    """lp (T, V) log-probabilities (rows t >= Tb are not read), the graph's arcs in stored order (sorted by dst) ->
    dict(n_hyp, hyp_score (K), hyp_len (K), hyp_arcs / hyp_tokens (K, max_len), paths = the whole arc tuples).  Every sum is
    taken in `dtype`, in the order the header states.  keys_seen: a dict that collects {key: history tuple} of every token
    made, for the check that hash identity is tuple identity."""
    lp = np.asarray(lp).astype(dtype)
    T, V = lp.shape
    Tb = max(min(int(Tb), T), 0)
    Q, A = int(num_nodes), len(src)
    max_len = T if max_len is None else int(max_len)
    src, dst, label, col = (np.asarray(x, dtype=np.int64) for x in (src, dst, label, col))
    w, final = np.asarray(w).astype(dtype), np.asarray(final).astype(dtype)
    colv = np.clip(label, 0, V - 1)
    incoming = [np.nonzero(dst == q)[0] for q in range(Q)]

    def extend(key, hist, a):
        ident = int(a) if distinct == ARCS else int(col[a])
        hist = hist + (ident,)
        key = mix(key, ident) if identity == "hash" else hist
        if keys_seen is not None:
            assert keys_seen.setdefault(key, hist) == hist, "two histories share a hash"
        return key, hist

    empty = 0 if identity == "hash" else ()
    # a token: (value, key, path, hist) - select_k reads the first two
    n = [[] for _ in range(Q)]
    n[0] = [(dtype(0), empty, (), ())]
    r = [[] for _ in range(A)]
    for t in range(Tb):
        nn, nr = [], []
        for q in range(Q):
            cands = list(n[q]) + [tok for a2 in incoming[q] for tok in r[a2]]
            nn.append([(lp[t, 0] + c[0],) + c[1:] for c in select_k(cands, K)])
        for a in range(A):
            s = src[a]
            E = select_k(list(n[s]) + [tok for a2 in incoming[s] if col[a2] != col[a] for tok in r[a2]], K)
            cands = list(r[a])
            for e in E:
                key, hist = extend(e[1], e[3], a)
                cands.append((e[0] + w[a], key, e[2] + (int(a),), hist))
            nr.append([(lp[t, colv[a]] + c[0],) + c[1:] for c in select_k(cands, K)])
        n = [[c for c in l if c[0] > -np.inf] for l in nn]
        r = [[c for c in l if c[0] > -np.inf] for l in nr]
    out = dict(n_hyp=0, hyp_score=np.full(K, -np.inf, dtype=dtype), hyp_len=np.full(K, -1, dtype=np.int32),
               hyp_arcs=np.full((K, max_len), -1, dtype=np.int32), hyp_tokens=np.full((K, max_len), -1, dtype=np.int32), paths=[])
    if Tb == 0:
        return out
    cands = []
    for q in range(Q):
        if final[q] > -np.inf:
            cands += [(c[0] + final[q],) + c[1:] for c in n[q]]
    for a in range(A):
        if final[dst[a]] > -np.inf:
            cands += [(c[0] + final[dst[a]],) + c[1:] for c in r[a]]
    for k, c in enumerate(select_k(cands, K)):
        path = c[2]
        out["hyp_score"][k], out["hyp_len"][k] = c[0], len(path)
        m = min(len(path), max_len)
        out["hyp_arcs"][k, :m] = path[:m]
        out["hyp_tokens"][k, :m] = label[list(path[:m])]
        out["paths"].append(path)
        out["n_hyp"] = k + 1
    return out


def nbest_graph(lp, Tb, g, K, distinct=ARCS, dtype=np.float32, identity="tuple", max_len=None, keys_seen=None):
    """nbest() on an openeat_amd.utils.decoding_graph.DecodingGraph."""
    return nbest(lp, Tb, g.num_nodes, g.src, g.dst, g.label, g.col, g.w, g.final, K, distinct, dtype, identity, max_len, keys_seen)


def path_score(lp, Tb, path, src, dst, label, w, final, dtype=np.float64):
    """The best-alignment score of one arc path: ctc_graph_ref.decode on its linear chain (-inf if it does not fit Tb frames or
    does not end in a final node)."""
    L = len(path)
    idx = list(path)
    end = int(dst[idx[-1]]) if L else 0
    fin = np.full(L + 1, -np.inf)
    fin[L] = final[end]
    lab = np.asarray(label)[idx] if L else np.zeros(0, dtype=np.int64)
    ww = np.asarray(w)[idx] if L else np.zeros(0)
    return R.decode(lp, Tb, L + 1, np.arange(L), np.arange(1, L + 1), lab, ww, fin, dtype)["score"]


def brute_force(lp, Tb, num_nodes, src, dst, label, w, final, distinct=ARCS, dtype=np.float64):
    """Every arc path from node 0 of at most Tb arcs that ends in a final node, each scored by path_score -> [(score, path)]
    sorted by score descending; with distinct == TOKENS only the best path of every label sequence."""
    T = np.asarray(lp).shape[0]
    Tb = max(min(int(Tb), T), 0)
    if Tb == 0:
        return []
    A = len(src)
    found = []
    stack = [((), 0)]
    while stack:
        path, node = stack.pop()
        if final[node] > -np.inf:
            sc = path_score(lp, Tb, path, src, dst, label, w, final, dtype)
            if sc > -np.inf:
                found.append((sc, path))
        if len(path) < Tb:
            for a in range(A):
                if int(src[a]) == node:
                    stack.append((path + (a,), int(dst[a])))
    if distinct == TOKENS:
        best = {}
        for sc, path in found:
            key = tuple(int(label[a]) for a in path)
            if key not in best or sc > best[key][0]:
                best[key] = (sc, path)
        found = list(best.values())
    return sorted(found, key=lambda x: -float(x[0]))
