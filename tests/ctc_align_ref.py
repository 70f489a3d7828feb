"""Float64, loop-level restatement of the CTC forced alignment that oe_ctc_align computes (the semantics are written out in
include/openeat_hip.h).  A helper for the alignment tests, not collected itself."""
import numpy as np

NEG = -np.inf


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def ext_labels(y):
    ext = [0]
    for c in y:
        ext += [int(c), 0]
    return ext


def collapse(path):
    """Merge repeats, drop blanks."""
    out, prev = [], None
    for c in path:
        c = int(c)
        if c != prev and c != 0:
            out.append(c)
        prev = c
    return out


def legal_move(ext, s_from, s_to):
    d = s_to - s_from
    if d in (0, 1):
        return True
    return d == 2 and s_to % 2 == 1 and s_to >= 3 and ext[s_to] != ext[s_to - 2]


def align(lp, y):
    """lp (Tb, V) log-probabilities, y the labels -> (score, state path, token path); (-inf, None, None) when no path exists.
    Ties: a predecessor replaces the best only if strictly greater, tried in the order stay, step, skip; the end state 2L is
    kept unless 2L-1 is strictly greater."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, ext = lp.shape[0], ext_labels(y)
    S = len(ext)
    if Tb == 0:
        return NEG, None, None
    v = np.full((Tb, S), NEG)
    bp = np.zeros((Tb, S), dtype=np.int64)
    v[0, 0] = lp[0, 0]
    if S > 1:
        v[0, 1] = lp[0, ext[1]]
    for t in range(1, Tb):
        for s in range(S):
            best, mv = v[t - 1, s], 0
            if s >= 1 and v[t - 1, s - 1] > best:
                best, mv = v[t - 1, s - 1], 1
            if s >= 3 and s % 2 == 1 and ext[s] != ext[s - 2] and v[t - 1, s - 2] > best:
                best, mv = v[t - 1, s - 2], 2
            v[t, s] = lp[t, ext[s]] + best
            bp[t, s] = mv
    s = S - 1
    if S > 1 and v[Tb - 1, S - 2] > v[Tb - 1, S - 1]:
        s = S - 2
    score = v[Tb - 1, s]
    if score == NEG:
        return NEG, None, None
    states = [0] * Tb
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= bp[t, s]
    return float(score), states, [ext[q] for q in states]


def path_score(lp, ext, states):
    return float(sum(np.asarray(lp, dtype=np.float64)[t, ext[s]] for t, s in enumerate(states)))


def spans(states, L):
    """First / last frame in state 2l+1 for every label l."""
    start, end = [-1] * L, [-1] * L
    for t, s in enumerate(states):
        if s % 2 == 1:
            if start[s >> 1] < 0:
                start[s >> 1] = t
            end[s >> 1] = t
    return start, end
