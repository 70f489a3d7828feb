"""The yardstick for the joint CTC/attention beam search with hotword biasing (openeat_amd/utils/joint_search.py states the
semantics): joint_lm_search_ref.joint_lm_search with one more summand and the extended pre-selection key, with or without
an LM, in plain Python / numpy.  Built from ctc_prefix_score_ref, joint_lm_search_ref and ctc_bias_beam_ref - whose hits /
pending / bias_direct are the bias BY DEFINITION, every end position and every phrase tried, no automaton - and independent
of openeat_amd.

A hypothesis g also carries b = bias(g) as it entered its total.  Candidate c has
    h' = hits(g . c),  b' = h' + float64(c) * k(g . c);   for <eos>: h' = b' = hits(g)  (the hypothesis ends, the pending credit
    is dropped; <eos> is not part of the prefix the graph sees),
    total = ((((1 - lam) a' + lam k') + beta len) [+ lm_weight m']) + b'
and the float32 key whose top-C (descending, ties to the lowest id) are the candidates is
    float32( l(v) [+ lm_weight * term(v), with an LM and lm_prebeam] [+ (b'(v) - b), with context_prebeam] ).
Without any summand beyond l the candidates are the decoder's own top-C.

The search returns the two gaps joint_lm_search_ref returns: the smallest relative gap between neighbouring totals at any
pruning and the smallest relative gap between the C-th and the (C+1)-th pre-selection key (inf where the key is l itself:
the device then cuts the very same float32 values).

Also here: the list of searches the GPU test runs and their graphs, shared with the CPU test that checks the gaps of every
one of them on the host."""
import itertools
import math

import numpy as np

import ctc_bias_beam_ref as B
import ctc_prefix_score_ref as ref
import joint_lm_search_ref as R

NEG = -math.inf


def ctx_next(graph, g, c, eos):
    """(hits', bias') of candidate c of hypothesis g (a token tuple without <eos>), from the definition."""
    if c == eos:
        h = B.bias(graph, g, True)
        return h, h
    p = tuple(g) + (c,)
    return B.bias(graph, p, True), B.bias(graph, p, False)


def joint_ctx_search(y, T, att_logp, eos, beam, C, ctc_weight, length_bonus, max_steps, graph, plm=None, lm_weight=0.0,
                     lm_prebeam=True, context_prebeam=True, blank=0):
    """The joint search of one utterance with the graph (ctc_bias_beam_ref.make_graph) and optionally the LM plm (a PrefixLM).
    Arguments as joint_lm_search_ref.joint_lm_search.
    -> (n-best [(tokens without <eos>, total, att, ctc, finished[, lm], bias)], totals' gap, pre-selection keys' gap)."""
    lam, beta, w = float(ctc_weight), float(length_bonus), float(lm_weight)
    hyps = [dict(g=(), a=0.0, k=0.0, m=0.0, b=0.0, fin=False, total=0.0, r=ref.empty_state(y, T, blank) if lam > 0 else None)]
    gap, key_gap = math.inf, math.inf
    lm_key = plm is not None and lm_prebeam
    for _ in range(max_steps):
        if all(h["fin"] for h in hyps):
            break
        cands = []
        for h in hyps:
            if h["fin"]:
                cands.append(h)
                continue
            lp = att_logp(h["g"])
            V = len(lp)
            if lm_key or context_prebeam:
                key = [float(lp[v]) for v in range(V)]
                if lm_key:
                    terms = [R.lm_term(plm, h["g"], v, eos) for v in range(V)]
                    key = [key[v] + w * terms[v] for v in range(V)]
                if context_prebeam:
                    key = [key[v] + (ctx_next(graph, h["g"], v, eos)[1] - h["b"]) for v in range(V)]
                key = [np.float32(x) for x in key]
                order = sorted(range(V), key=lambda v: (-float(key[v]), v))
                if V > C:
                    key_gap = min(key_gap, R.rel_gap(float(key[order[C - 1]]), float(key[order[C]])))
                chosen = order[:C]
            else:
                chosen = ref.top_candidates(lp, C)
            for c in chosen:
                a = h["a"] + float(lp[c])
                m = h["m"] + R.lm_term(plm, h["g"], c, eos) if plm is not None else 0.0
                b = ctx_next(graph, h["g"], c, eos)[1]
                fin = c == eos
                g = h["g"] + (c,)
                n = len(g) - (1 if fin else 0)
                k, r = 0.0, None
                if lam > 0:
                    k, r = ref.prefix_score(y, T, h["r"], h["g"], c, eos, blank)
                    total = ((1.0 - lam) * a + lam * k) + beta * n
                else:
                    total = (1.0 - lam) * a + beta * n
                if plm is not None:
                    total = total + w * m
                total = total + b
                if total == NEG:
                    continue
                cands.append(dict(g=g, a=a, k=k, m=m, b=b, fin=fin, total=total, r=r))
        cands.sort(key=lambda h: -h["total"])                                # stable: ties stay in (slot, rank) order
        for p, q in zip(cands, cands[1:]):
            gap = min(gap, R.rel_gap(p["total"], q["total"]))
        hyps = cands[:beam]
        if not hyps:
            break
    out = [h for h in hyps if h["fin"]] + [h for h in hyps if not h["fin"]]
    rows = [(list(h["g"][:-1] if h["fin"] else h["g"]), h["total"], h["a"], h["k"], h["fin"]) + (() if plm is None else (h["m"],)) + (h["b"],)
            for h in out]
    return rows, gap, key_gap


def yardstick(y, tab, lens, graph, plm, beam, C, lam, beta, max_steps, lm_weight, lm_prebeam, context_prebeam):
    """Per utterance (n-best, totals' gap, keys' gap) for the table-driven scorer of joint_lm_search_ref.make_case_host."""
    y64, V, steps = y.astype(np.float64), y.shape[2], tab.shape[1] - 1
    out = []
    for u in range(y.shape[0]):
        att = lambda g, u=u: tab[u, min(len(g), steps), (g[-1] + 1) if g else 0]     # noqa: E731
        out.append(joint_ctx_search(y64[u], int(lens[u]), att, V - 1, beam, C, lam, beta, max_steps, graph, plm, lm_weight, lm_prebeam,
                                    context_prebeam))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases: the shapes, weights and LM of joint_lm_search_ref, tables and graphs of their own seeds
SHAPES = R.SHAPES                                                      # (B, Tmax, V, lens, ...): B <= 3, Tmax <= 23, V <= 12
TABLE_SEED = {"small": 31, "mid": 32, "survivor": R.SURVIVOR["seed"]}
GRAPH_SEED = 5
LM_ORDER = 2
# None: no LM; otherwise (order, lm_prebeam)
LM_MODES = (None, (LM_ORDER, True), (LM_ORDER, False))
N_FIRE, N_RANDOM = 5, 5


def make_tables(shape):
    """make_case_host of a shape (or "survivor") with this file's seed -> (y, tab, lens)."""
    if shape == "survivor":
        c = R.SURVIVOR
        return R.make_case_host(c["B"], c["Tmax"], c["V"], TABLE_SEED[shape], **c["kw"]) + (c["lens"],)
    Bn, Tmax, V, lens, _ = SHAPES[shape]
    return R.make_case_host(Bn, Tmax, V, TABLE_SEED[shape]) + (lens,)


def case_graph(shape, y, tab, lens):
    """The graph of a shape, the same on every machine: N_FIRE sub-sequences of the un-biased n-best (they fire) and N_RANDOM
    random phrases (they mostly fail midway) over the tokens 1 .. V-2, explicit scores that do not sum exactly in float32,
    c = ctc_bias_beam_ref.C."""
    V, Tmax = y.shape[2], y.shape[1]
    rng = np.random.default_rng(GRAPH_SEED + V)
    empty = B.make_graph([], 0.0)
    nbest = [[tuple(h[0]) for h in nb] for nb, _, _ in yardstick(y, tab, lens, empty, None, 3, 4, 0.3, 0.0, Tmax, 0.0, True, False)]
    phrases = B.phrases_for(nbest, V - 1, N_FIRE, N_RANDOM, rng, max_len=4)
    scores = rng.uniform(0.2, 2.5, len(phrases)).astype(np.float32)
    return B.make_graph(phrases, B.C, scores)


def survivor_graph(V):
    """The graph of the SURVIVOR case: every token is a phrase of its own, so whatever a finished hypothesis' slot were extended
    by would change its bias."""
    return B.make_graph([(t,) for t in range(1, V - 1)], 0.25, [0.3 + 0.1 * t for t in range(1, V - 1)])


def search_cases():
    """Every search of test_search_loop_against_the_yardstick: (shape, lam, beam, lm_weight, context_prebeam, lm mode)."""
    return list(itertools.product(SHAPES, R.LAMS, R.BEAMS, R.WEIGHTS, (True, False), LM_MODES))
