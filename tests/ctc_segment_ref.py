"""Float64 restatement of the long-form CTC segmentation that oe_ctc_segment computes (the semantics are written out in
include/openeat_hip.h): a loop over frames, vectorised over states.  A helper for the segmentation tests, not collected itself."""
import numpy as np

from ctc_align_ref import NEG, ext_labels


def skip_mask(ext):
    """allowed[s]: the move s-2 -> s exists (odd s >= 3 between different labels)."""
    e = np.asarray(ext)
    ok = np.zeros(len(e), dtype=bool)
    if len(e) >= 4:
        s = np.arange(3, len(e), 2)
        ok[s] = e[s] != e[s - 2]
    return ok


def segment(lp, y, free_start, free_end):
    """lp (Tb, V) log-probabilities, y the labels -> (score, state path); (-inf, None) when no path exists.  Ties as in
    ctc_align_ref.align: a predecessor replaces the best only if strictly greater, tried in the order stay, step, skip; the end
    state 2L is kept unless 2L-1 is strictly greater."""
    lp = np.asarray(lp, dtype=np.float64)
    Tb, ext = lp.shape[0], np.asarray(ext_labels(y))
    S, L = len(ext), len(y)
    if Tb == 0:
        return NEG, None
    skip = skip_mask(ext)
    v = np.full(S, NEG)
    v[0] = 0.0 if free_start else lp[0, 0]
    if S > 1:
        v[1] = lp[0, ext[1]]
    bp = np.zeros((Tb, S), dtype=np.int8)
    end_free = free_end and not (free_start and L == 0)
    for t in range(1, Tb):
        best, mv = v.copy(), np.zeros(S, dtype=np.int8)
        step = np.concatenate([[NEG], v])[:S]
        m = step > best
        best[m], mv[m] = step[m], 1
        sk = np.concatenate([[NEG, NEG], v])[:S]
        m = skip & (sk > best)
        best[m], mv[m] = sk[m], 2
        nv = best + lp[t, ext]
        if end_free:                                     # staying in 2L is free, entering it costs the blank
            stay, ent = v[S - 1], (v[S - 2] + lp[t, 0] if S > 1 else NEG)
            nv[S - 1], mv[S - 1] = (ent, 1) if ent > stay else (stay, 0)
        if free_start:
            nv[0], mv[0] = 0.0, 0
        v, bp[t] = nv, mv
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    if v[s] == NEG:
        return NEG, None
    states = [0] * Tb
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return float(v[states[-1]]), states


def free_frames(states, L, free_start, free_end):
    """free[t]: frame t of the path costs nothing."""
    st = np.asarray(states)
    fr = np.zeros(len(st), dtype=bool)
    if free_start:
        fr |= st == 0
    if free_end:
        fr[1:] |= (st[1:] == 2 * L) & (st[:-1] == 2 * L)
    return fr


def path_score(lp, ext, states, free_start, free_end):
    """Float64 sum, in frame order, of lp[t, ext[state_t]] over the frames of the path that are not free."""
    lp = np.asarray(lp, dtype=np.float64)
    L = (len(ext) - 1) // 2
    fr = free_frames(states, L, free_start, free_end)
    return float(sum(lp[t, ext[s]] for t, s in enumerate(states) if not fr[t]))


def plant(rng, T, y, p_blank=0.5, head=0, tail=0, first_one=False):
    """A random legal state path of T frames through y: `head` frames in state 0, a core that begins and ends with one
    blank frame (states 0 and 2L) and visits every label, `tail` more frames in state 2L.  Between two labels the blank is
    visited with probability p_blank (always between equal labels); the frames left over are spread as repeats over the
    core's visits (none on the first label with first_one: it occupies exactly one frame).  None if T is too short."""
    L = len(y)
    visits = [0]
    for l in range(L):
        if l > 0 and (y[l] == y[l - 1] or rng.random() < p_blank):
            visits.append(2 * l)
        visits.append(2 * l + 1)
    if L > 0:
        visits.append(2 * L)
    spare = T - head - tail - len(visits)
    if spare < 0:
        return None
    reps = np.ones(len(visits), dtype=np.int64)
    ok = np.array([not (first_one and s == 1) for s in visits])
    ok[0] = ok[-1] = False                                # one blank frame at either end of the core
    if spare and ok.any():
        reps += np.bincount(rng.choice(np.flatnonzero(ok), size=spare), minlength=len(visits))
    elif spare:
        head += spare
    return [0] * head + [s for s, r in zip(visits, reps) for _ in range(int(r))] + [2 * L] * tail


def planted_case(rng, T, V, y, free_start, free_end, junk, p_blank=0.5, margin=3):
    """Logits whose best path is planted: float32 randn with +8 on the planted path's token; under a free flag a head / tail
    of `margin` .. margin + 5 junk frames whose +8 sits on an id drawn from `junk` (ids no label uses).  The first label
    occupies exactly one frame (see the header: under free_start the path leaves state 0 as late as it can).
    -> (logits (T, V) float32, states) or None if T is too short."""
    head = int(rng.integers(margin, margin + 6)) if free_start else 0
    tail = int(rng.integers(margin, margin + 6)) if free_end else 0
    states = plant(rng, T, y, p_blank, head, tail, first_one=True)
    if states is None:
        return None
    ext = np.asarray(ext_labels(y))
    tok = ext[np.asarray(states)]
    tok[:head] = rng.choice(junk, size=head)
    if tail:
        tok[T - tail:] = rng.choice(junk, size=tail)
    logits = rng.standard_normal((T, V), dtype=np.float32)
    logits[np.arange(T), tok] += 8.0
    return logits, states
