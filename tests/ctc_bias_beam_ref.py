"""The yardstick for the hotword-biased CTC prefix beam search: the dict loop of ctc_lm_beam_ref.search with one more
summand in the key that orders next_hyps,

    total(p) = ((log_add(pb, pnb) + lm_weight * LM(p)) + length_bonus * len(p)) + bias(p)          (no LM: no LM term)
    bias(p)  = hits(p) + float64(c) * k(p);  with `final`, at the end of the utterance, bias(p) = hits(p)

and the bias computed by BRUTE FORCE from the declarative definition (include/openeat_hip.h): every end position and every
phrase is tried for hits(p), every suffix length for k(p).  No automaton, nothing of openeat_amd.

    hits(p) = sum of s(q) over the occurrences (i, q), p[i-len(q):i] == q - the float32 scores added in float64 by increasing
              i, the longest phrase first within one i;
    k(p)    = the largest k <= len(p) such that p's last k tokens are a proper prefix of some phrase (0: none).

A graph here is (phrases: list of token tuples, scores: list of float32, c: float32, memo); the memo keeps (hits, k) per
prefix, so that the runs of one case share them."""
import math

import numpy as np

from ctc_lm_beam_ref import CASES, NEG, PrefixLM, _gap, log_add, make_case  # noqa: F401 - the cases travel with the yardstick


def make_graph(phrases, c, scores=None):
    """-> (phrases as tuples, float32 scores (default: c * len in float32), float32 c, an empty memo)."""
    phrases = [tuple(int(t) for t in q) for q in phrases]
    c = np.float32(c)
    scores = [c * np.float32(len(q)) for q in phrases] if scores is None else [np.float32(s) for s in scores]
    return phrases, scores, c, {}


def hits(graph, prefix):
    phrases, scores = graph[:2]
    prefix = tuple(prefix)
    by_length = sorted(range(len(phrases)), key=lambda n: -len(phrases[n]))          # stable: the longest phrase first
    h = 0.0
    for i in range(1, len(prefix) + 1):
        for n in by_length:
            q = phrases[n]
            if len(q) <= i and prefix[i - len(q):i] == q:
                h += float(scores[n])
    return h


def pending(graph, prefix):
    phrases = graph[0]
    prefix = tuple(prefix)
    longest = max([len(q) for q in phrases] + [0])
    for k in range(min(len(prefix), longest - 1), 0, -1):              # a proper prefix is shorter than its phrase
        tail = prefix[len(prefix) - k:]
        if any(len(q) > k and q[:k] == tail for q in phrases):
            return k
    return 0


def bias_direct(graph, prefix, final=False):
    """bias(p) from the whole prefix, nothing remembered."""
    h = hits(graph, prefix)
    return h if final else h + float(graph[2]) * pending(graph, prefix)


def _hits_k(graph, prefix):
    """(hits, k) through the memo.  hits(p) is hits(p[:-1]) - the positions i < len(p), already added in order - plus the
    phrases that end at i = len(p), every one of them tried, the longest first: the same additions in the same order as
    hits() makes (tests/test_ctc_bias_beam_ref.py compares the two)."""
    v = graph[3].get(prefix)
    if v is None:
        h = 0.0
        if prefix:
            h = _hits_k(graph, prefix[:-1])[0]
            phrases, scores = graph[:2]
            for n in sorted(range(len(phrases)), key=lambda n: -len(phrases[n])):
                q = phrases[n]
                if len(q) <= len(prefix) and prefix[len(prefix) - len(q):] == q:
                    h += float(scores[n])
        v = graph[3][prefix] = (h, pending(graph, prefix))
    return v


def bias(graph, prefix, final=False):
    h, k = _hits_k(graph, tuple(prefix))
    return h if final else h + float(graph[2]) * k


class _NoLM:
    def lm(self, prefix):
        return 0.0


def search(top_logp, top_idx, beam, graph, plm=None, lm_weight=0.0, length_bonus=0.0, eos=True, final=True):
    """As ctc_lm_beam_ref.search; plm None: no LM -> ([(prefix, total, ctc, lm, bias)] sorted by total, smallest non-zero
    relative gap); lm is 0.0 without an LM."""
    def running_bias(prefix):
        return bias(graph, prefix)

    def total(prefix, ctc, lm, b):
        if plm is None:
            return (ctc + length_bonus * len(prefix)) + b
        return ((ctc + lm_weight * lm) + length_bonus * len(prefix)) + b

    lmof = plm if plm is not None else _NoLM()
    cur = [((), (0.0, NEG))]
    gap = math.inf
    for t in range(len(top_idx)):
        nxt = {}
        for j in range(len(top_idx[t])):
            s, ps = int(top_idx[t][j]), float(top_logp[t][j])
            for prefix, (pb, pnb) in cur:
                last = prefix[-1] if prefix else None
                if s == 0:
                    a, b = nxt.get(prefix, (NEG, NEG))
                    nxt[prefix] = (log_add([a, pb + ps, pnb + ps]), b)
                elif s == last:
                    a, b = nxt.get(prefix, (NEG, NEG))
                    nxt[prefix] = (a, log_add([b, pnb + ps]))
                    ext = prefix + (s,)
                    a, b = nxt.get(ext, (NEG, NEG))
                    nxt[ext] = (a, log_add([b, pb + ps]))
                else:
                    ext = prefix + (s,)
                    a, b = nxt.get(ext, (NEG, NEG))
                    nxt[ext] = (a, log_add([b, pb + ps, pnb + ps]))
        keyed = [(total(p, log_add(list(v)), lmof.lm(p), running_bias(p)), p, v) for p, v in nxt.items()]       # insertion order
        keyed.sort(key=lambda e: e[0], reverse=True)                                                          # stable
        gap = _gap([e[0] for e in keyed], beam, gap)
        cur = [(p, v) for _, p, v in keyed[:beam]]
    out = []
    for prefix, (pb, pnb) in cur:
        ctc = log_add([pb, pnb])
        lm = lmof.lm(prefix)
        if eos and plm is not None:
            lm = lm + plm.eos(prefix)
        b = bias(graph, prefix, final)
        out.append((prefix, total(prefix, ctc, lm, b), ctc, lm, b))
    out.sort(key=lambda h: h[1], reverse=True)
    gap = _gap([h[1] for h in out], beam, gap)
    return out, gap


def phrases_for(nbest, V, n_fire, n_random, rng, max_len=6):
    """Distinct phrases for a test graph: n_fire sub-sequences of the given n-best prefixes (they fire) and n_random random
    token sequences (they mostly fail midway)."""
    seen, out = set(), []
    pool = [p for nb in nbest for p in nb if len(p) >= 1]
    tries = 0
    while len(out) < n_fire and pool and tries < 50 * n_fire:
        tries += 1
        p = pool[int(rng.integers(0, len(pool)))]
        n = int(rng.integers(1, min(max_len, len(p)) + 1))
        i = int(rng.integers(0, len(p) - n + 1))
        q = tuple(p[i:i + n])
        if q not in seen:
            seen.add(q)
            out.append(q)
    tries = 0
    target = len(out) + n_random
    while len(out) < target and tries < 50 * n_random:
        tries += 1
        q = tuple(int(t) for t in rng.integers(1, V, int(rng.integers(2, max_len + 1))))
        if q not in seen:
            seen.add(q)
            out.append(q)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the random cases: those of ctc_lm_beam_ref (CASES, make_case), each with a graph drawn from its own unbiased n-best
C = 0.37                                                               # not dyadic: c * k is rounded
WEIGHTS = [(0.5, 0.0), (0.3, 0.8)]                                     # (lm_weight, length_bonus); no LM: the bonus alone
N_PHRASES = 12


def cpu_topk(logits, beam):
    """Per frame the `beam` largest log-probabilities, ties to the lowest index (as ops.topk_rows orders them)."""
    import torch
    lp = torch.log_softmax(logits, -1).numpy()
    idx = np.argsort(-lp, axis=-1, kind="stable")[..., :beam]
    return np.take_along_axis(lp, idx, -1), idx.astype(np.int64)


def case_graph(logits, lens, V, beam, seed=0):
    """The graph of a random case, the same on every machine: half of the phrases are sub-sequences of the unbiased n-best on
    the CPU's log_softmax top-k (they fire), half are random (they fail midway); explicit scores, c = C."""
    rng = np.random.default_rng(1000 + seed + V + beam)
    tp, ti = cpu_topk(logits, beam)
    empty = make_graph([], 0.0)
    nbest = [[h[0] for h in search(tp[b, : lens[b]], ti[b, : lens[b]], beam, empty)[0]] for b in range(len(lens))]
    phrases = phrases_for(nbest, V, N_PHRASES // 2, N_PHRASES // 2, rng)
    scores = rng.uniform(0.2, 2.5, len(phrases)).astype(np.float32)
    return make_graph(phrases, C, scores)
