"""Numpy float64 restatement of the CTC prefix score and of the joint CTC/attention beam search (the semantics are written
out in include/openeat_hip.h at oe_ctc_prefix_score and in openeat_amd/utils/joint_search.py), written from those equations and
independent of the product: the recursion, the per-utterance search over a callable that gives the attention
log-probabilities, and a brute-force prefix probability that enumerates every alignment."""
import itertools
import math

import numpy as np

NEG = -math.inf


def log_add(a, b):
    if a == NEG and b == NEG:
        return NEG
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def empty_state(y, T, blank=0):
    """r (T, 2) of the empty hypothesis: column 0 non-blank, column 1 blank."""
    r = np.full((T, 2), NEG, dtype=np.float64)
    acc = 0.0
    for t in range(T):
        acc += float(y[t, blank])
        r[t, 1] = acc
    return r


def prefix_score(y, T, r, g, c, eos, blank=0):
    """psi(g . c) and the state of g . c (None where no state is produced) from g's state r (T, 2)."""
    V = y.shape[1]
    if c == blank or not 0 <= c < V:
        return NEG, None
    if T == 0:
        return (0.0 if c == eos and len(g) == 0 else NEG), None
    if c == eos:
        return log_add(float(r[T - 1, 0]), float(r[T - 1, 1])), None
    n = np.full((T, 2), NEG, dtype=np.float64)
    n[0, 0] = float(y[0, c]) if len(g) == 0 else NEG
    psi = float(n[0, 0])
    for t in range(1, T):
        phi = float(r[t - 1, 1]) if len(g) > 0 and c == g[-1] else log_add(float(r[t - 1, 0]), float(r[t - 1, 1]))
        n[t, 0] = log_add(float(n[t - 1, 0]), phi) + float(y[t, c])
        n[t, 1] = log_add(float(n[t - 1, 0]), float(n[t - 1, 1])) + float(y[t, blank])
        psi = log_add(psi, phi + float(y[t, c]))
    return psi, n


def state_of(y, T, g, eos, blank=0):
    """The state of the hypothesis g, built one extension at a time."""
    r = empty_state(y, T, blank)
    for i, c in enumerate(g):
        _, r = prefix_score(y, T, r, tuple(g[:i]), c, eos, blank)
        assert r is not None, "a hypothesis holds neither blank nor <eos> nor an id outside the vocabulary"
    return r


def full_likelihood(y, T, g, eos, blank=0):
    """log p_ctc(g | y): what <eos> after g scores."""
    if T == 0:
        return 0.0 if len(g) == 0 else NEG
    return prefix_score(y, T, state_of(y, T, g, eos, blank), tuple(g), eos, eos, blank)[0]


def collapse(path, blank=0):
    out, prev = [], None
    for k in path:
        if k != blank and k != prev:
            out.append(k)
        prev = k
    return tuple(out)


def brute_force(y, T, h, blank=0):
    """(log-probability that the label sequence starts with h, log-probability that it is exactly h, the state of h as a
    (T, 2) array) by enumerating all V^T alignments (and, for the state, all V^(t+1) of every shorter stretch)."""
    V = y.shape[1]
    h = tuple(h)
    p = np.exp(np.asarray(y, dtype=np.float64))
    starts = exact = 0.0
    for path in itertools.product(range(V), repeat=T):
        w = 1.0
        for t, k in enumerate(path):
            w *= p[t, k]
        lab = collapse(path, blank)
        if lab[:len(h)] == h:
            starts += w
        if lab == h:
            exact += w
    state = np.zeros((T, 2))
    for t in range(T):
        for path in itertools.product(range(V), repeat=t + 1):
            if collapse(path, blank) == h:
                w = 1.0
                for s, k in enumerate(path):
                    w *= p[s, k]
                state[t, 1 if path[-1] == blank else 0] += w
    lg = lambda v: math.log(v) if v > 0 else NEG                           # noqa: E731
    return lg(starts), lg(exact), np.vectorize(lg)(state) if T else state


def top_candidates(logp, C):
    """The C best token ids, descending, ties to the lowest id (the order of oe_topk_rows)."""
    return sorted(range(len(logp)), key=lambda v: (-float(logp[v]), v))[:C]


def joint_search(y, T, att_logp, eos, beam, C, ctc_weight, length_bonus, max_steps, blank=0):
    """The joint search of one utterance.  y (>= T, V) CTC log-probabilities, att_logp(g) -> (V) attention log-probabilities
    after the hypothesis g (a tuple, without <sos>).  -> (n-best [(tokens without <eos>, total, att, ctc, finished)],
    smallest non-zero gap between neighbouring totals at any pruning).  With ctc_weight == 0 no CTC score is formed: ctc is 0."""
    lam, beta = float(ctc_weight), float(length_bonus)
    hyps = [dict(g=(), a=0.0, k=0.0, fin=False, total=0.0, r=empty_state(y, T, blank) if lam > 0 else None)]
    gap = math.inf
    for _ in range(max_steps):
        if all(h["fin"] for h in hyps):
            break
        cands = []
        for h in hyps:
            if h["fin"]:
                cands.append(h)
                continue
            lp = att_logp(h["g"])
            for c in top_candidates(lp, C):
                a = h["a"] + float(lp[c])
                fin = c == eos
                g = h["g"] + (c,)
                total = (1.0 - lam) * a + beta * (len(g) - (1 if fin else 0))
                k, r = 0.0, None
                if lam > 0:
                    k, r = prefix_score(y, T, h["r"], h["g"], c, eos, blank)
                    total = (1.0 - lam) * a + lam * k + beta * (len(g) - (1 if fin else 0))
                if total == NEG:
                    continue
                cands.append(dict(g=g, a=a, k=k, fin=fin, total=total, r=r))
        cands.sort(key=lambda h: -h["total"])                                # stable: ties stay in (slot, rank) order
        for p, q in zip(cands, cands[1:]):
            if p["total"] > q["total"]:
                gap = min(gap, p["total"] - q["total"])
        hyps = cands[:beam]
        if not hyps:
            break
    out = [h for h in hyps if h["fin"]] + [h for h in hyps if not h["fin"]]
    return [(list(h["g"][:-1] if h["fin"] else h["g"]), h["total"], h["a"], h["k"], h["fin"]) for h in out], gap
