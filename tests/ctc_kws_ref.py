"""Loop-level restatement of the keyword search over CTC posteriors that oe_ctc_kws computes (the semantics are written out in
include/openeat_hip.h): the recursion with carried start frames, the candidates, the exact cross-multiplied comparisons and
the pending-hit scan.  float64 by default; `dtype` runs the same code with the recursion's values in float32 (comparisons
between candidates are in float64 either way, as the header has them).  Reachability is a flag of its own here, so nothing
depends on a stand-in for -inf.  A helper for the keyword-search tests, not collected itself."""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def columns(y, V):
    """The column of lp every state 1 .. 2L-1 reads (a label outside [0, V) reads the nearest valid column) and whether the
    skip into it is legal (odd s >= 3 whose label differs, as given, from the label two states back)."""
    n = 2 * len(y) - 1
    col = np.zeros(n, dtype=np.int64)
    skip = np.zeros(n, dtype=bool)
    for j in range(n):
        s = j + 1
        if s & 1:
            col[j] = min(max(int(y[s >> 1]), 0), V - 1)
            skip[j] = s >= 3 and int(y[s >> 1]) != int(y[(s >> 1) - 1])
    return col, skip


def better(a_sc, a_n, b_sc, b_n):
    """a is better than b: a larger mean log-probability per frame, compared exactly without a division."""
    return float(a_sc) * int(b_n) > float(b_sc) * int(a_n)


def passes(sc, n, thr):
    return float(sc) >= float(thr) * int(n)


def candidates(lp, y, dtype=np.float64):
    """lp (Tb, V) log-probabilities -> [(t, st, sc)] for every frame t at which state 2L-1 is reachable: the value of the
    best path that spells y and ends at t with its start free, and the frame st at which that path entered state 1."""
    lp = np.asarray(lp, dtype=dtype)
    Tb, V = lp.shape
    L = len(y)
    if L == 0 or Tb == 0:
        return []
    col, skip = columns(y, V)
    n = 2 * L - 1
    v = np.zeros(n, dtype=dtype)
    st = np.full(n, -1, dtype=np.int64)
    reach = np.zeros(n, dtype=bool)
    out = []
    for t in range(Tb):
        best, bst, br = v.copy(), st.copy(), reach.copy()
        # step, then skip: a predecessor replaces the best only if strictly greater (or the best does not exist)
        for d in (1, 2):
            pv, ps, pr = np.zeros(n, dtype=dtype), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=bool)
            pv[d:], ps[d:], pr[d:] = v[:n - d], st[:n - d], reach[:n - d]
            if d == 2:
                pr &= skip
            take = pr & (~br | (pv > best))
            best, bst, br = np.where(take, pv, best), np.where(take, ps, bst), br | take
        if not br[0] or dtype(0) > best[0]:                    # fresh, state 1 only
            best[0], bst[0], br[0] = 0, t, True
        v = np.where(br, best + lp[t, col], dtype(0)).astype(dtype)
        st, reach = bst, br
        if reach[n - 1]:
            out.append((t, int(st[n - 1]), dtype(v[n - 1])))
    return out


def scan(cands, thr):
    """The pending-hit scan over the candidates of one (recording, keyword) -> (hits [(st, en, sc)] in time order, best
    (st, en, sc) or None)."""
    hits, pend, best = [], None, None
    for t, st, sc in cands:
        n = t - st + 1
        if best is None or better(sc, n, best[2], best[1] - best[0] + 1):
            best = (st, t, sc)
        if not passes(sc, n, thr):
            continue
        if pend is not None and st <= pend[1]:
            if better(sc, n, pend[2], pend[1] - pend[0] + 1):
                pend = (st, t, sc)
        else:
            if pend is not None:
                hits.append(pend)
            pend = (st, t, sc)
    if pend is not None:
        hits.append(pend)
    return hits, best


def search_one(lp, y, thr, dtype=np.float64):
    return scan(candidates(lp, y, dtype), thr)


def search(lp, hlens, keywords, thr, max_hits, dtype=np.float64):
    """lp (B, T, V) log-probabilities, keywords a list of label lists (an empty one has no hits), thr (K) as the device reads it
    (float32 values) -> the device's outputs as numpy arrays: n_hits (B, K) int32, hit_start / hit_end (B, K, max_hits) int32,
    hit_score (B, K, max_hits) float32, best_start / best_end (B, K) int32, best_score (B, K) float32."""
    B, K = len(hlens), len(keywords)
    n_hits = np.zeros((B, K), dtype=np.int32)
    hs = np.full((B, K, max_hits), -1, dtype=np.int32)
    he = np.full((B, K, max_hits), -1, dtype=np.int32)
    hv = np.zeros((B, K, max_hits), dtype=np.float32)
    bs = np.full((B, K), -1, dtype=np.int32)
    be = np.full((B, K), -1, dtype=np.int32)
    bv = np.full((B, K), -np.inf, dtype=np.float32)
    for b in range(B):
        Tb = int(hlens[b])
        for k, y in enumerate(keywords):
            hits, best = search_one(np.asarray(lp[b])[:Tb], y, thr[k], dtype)
            n_hits[b, k] = len(hits)
            for i, (s, e, sc) in enumerate(hits[:max_hits]):
                hs[b, k, i], he[b, k, i], hv[b, k, i] = s, e, sc
            if best is not None:
                bs[b, k], be[b, k], bv[b, k] = best
    return n_hits, hs, he, hv, bs, be, bv


def span_optimum(lp, y, a, t):
    """float64: the best path that begins in state 1 at frame a and ends in state 2L-1 at frame t (-inf if none)."""
    lp = np.asarray(lp, dtype=np.float64)
    col, skip = columns(y, lp.shape[1])
    n = 2 * len(y) - 1
    v = np.full(n, -np.inf)
    v[0] = lp[a, col[0]]
    for f in range(a + 1, t + 1):
        best = v.copy()
        best[1:] = np.maximum(best[1:], v[:-1])
        if n > 2:
            best[2:] = np.maximum(best[2:], np.where(skip[2:], v[:-2], -np.inf))
        v = best + lp[f, col]
    return float(v[n - 1])


def grid_case(rng, T, V, zero_p=0.5):
    """(T, V) values drawn from the multiples of 1/8 in [-3, 0], about half of them 0: every float32 sum of them is exact, and
    ties are everywhere."""
    x = -rng.integers(0, 25, size=(T, V)).astype(np.float64) / 8
    x[rng.random((T, V)) < zero_p] = 0.0
    return x


def continuous_case(seed, T, V, keywords, n_plant=4, boost=14.0):
    """N(0, 4) logits (T, V) with n_plant occurrences of keywords planted (every frame of an occurrence raised by `boost` on its
    path: each label held 1 - 3 frames and the last one a single frame, a blank between labels half of the time and always
    between equal ones) -> (logits float32, [(keyword index, first frame, last frame)]) - the span the search returns for a
    planted occurrence is the tight one: from the last frame of its first label's run to the frame of its last label."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((T, V)) * 2).astype(np.float32)
    planted, t = [], int(rng.integers(2, 8))
    for i in range(n_plant):
        k = int(rng.integers(0, len(keywords)))
        y = keywords[k]
        if not y:
            continue
        runs = []
        for j, c in enumerate(y):
            if j and (y[j - 1] == c or rng.random() < 0.5):
                runs.append((0, int(rng.integers(1, 3))))
            runs.append((int(c), 1 if j == len(y) - 1 else int(rng.integers(1, 4))))
        if t + sum(r for _, r in runs) + 8 > T:
            break
        first_end = t + runs[0][1] - 1
        for c, r in runs:
            logits[t:t + r, c] += boost
            last_start = t
            t += r
        planted.append((k, first_end, last_start))
        t += int(rng.integers(6, 14))
    return logits, planted


RAW_SEEDS = list(range(100, 110))       # the continuous fixtures: test_ctc_kws_ref.py holds every one to the float32 == float64 condition


def raw_keywords(V=40, K=70, seed=3):
    rng = np.random.default_rng(seed)
    kws = [[int(c) for c in rng.integers(1, V, size=int(rng.integers(2, 7)))] for _ in range(K)]
    kws[1][1] = kws[1][0]                                   # one adjacent repeat
    return kws


def raw_fixture(seed, V=40, K=70):
    """(logits (T, V) float32 with T = 600 for even seeds and 300 for odd ones, the K keywords of 2 - 6 labels, the planted
    occurrences)."""
    kws = raw_keywords(V, K)
    logits, planted = continuous_case(seed, 300 if seed % 2 else 600, V, kws, n_plant=6)
    return logits, kws, planted
