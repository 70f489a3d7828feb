"""The yardstick for the joint CTC/attention beam search with n-gram LM fusion (openeat_amd/utils/joint_search.py states the
semantics): ctc_prefix_score_ref.joint_search with the LM term and both pre-selection modes, in plain Python / numpy, built
from ctc_prefix_score_ref's functions and ctc_lm_beam_ref.PrefixLM / ngram_ref.RefLM and independent of openeat_amd.

A hypothesis also carries m, the left-to-right float64 sum of its tokens' LM terms (log10; the </s> term for <eos>), and
    total = (((1 - lam) a' + lam k') + beta len) + lm_weight m'
Pre-selection: with lm_prebeam the C candidates of a hypothesis are the top-C tokens (descending, ties to the lowest id) of the
float32 key  float32(l(v) + lm_weight * term(v)); without it they are the decoder's own top-C.

RefLM.p sums a term right to left (the shortest context's back-off first), the kernel left to right: the two can differ in
the last bit.  So the search also returns two gaps per utterance, which make a comparison with the device sound - the
smallest relative gap between neighbouring totals at any pruning (a tie counts as a gap of 0), and the smallest relative gap
between the C-th and the (C+1)-th float32 pre-selection key of any live hypothesis.

Also here: the generator of the test cases and the list of searches the GPU test runs, shared with the CPU test that checks
the gaps of every one of them on the host."""
import itertools
import math

import numpy as np

import ctc_prefix_score_ref as ref
import ngram_ref
from ctc_lm_beam_ref import PrefixLM

NEG = -math.inf


def lm_term(plm, g, c, eos):
    """log10 p(c | <s> g): the </s> term for <eos>."""
    return plm.eos(tuple(g)) if c == eos else plm.ref.p(plm.word(c), plm.context(tuple(g)))[0]


def rel_gap(a, b):
    return (a - b) / max(1.0, abs(a))


def joint_lm_search(y, T, att_logp, eos, beam, C, ctc_weight, length_bonus, max_steps, plm, lm_weight, lm_prebeam=True, blank=0):
    """The joint search of one utterance with the LM plm (a PrefixLM).  Arguments as ctc_prefix_score_ref.joint_search.
    -> (n-best [(tokens without <eos>, total, att, ctc, finished, lm)], totals' gap, pre-selection keys' gap)."""
    lam, beta, w = float(ctc_weight), float(length_bonus), float(lm_weight)
    hyps = [dict(g=(), a=0.0, k=0.0, m=0.0, fin=False, total=0.0, r=ref.empty_state(y, T, blank) if lam > 0 else None)]
    gap, key_gap = math.inf, math.inf
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
            if lm_prebeam:
                terms = [lm_term(plm, h["g"], v, eos) for v in range(V)]
                key = [np.float32(float(lp[v]) + w * terms[v]) for v in range(V)]
                order = sorted(range(V), key=lambda v: (-float(key[v]), v))
                if V > C:
                    key_gap = min(key_gap, rel_gap(float(key[order[C - 1]]), float(key[order[C]])))
                chosen = order[:C]
            else:
                chosen = ref.top_candidates(lp, C)
                terms = {c: lm_term(plm, h["g"], c, eos) for c in chosen}
            for c in chosen:
                a = h["a"] + float(lp[c])
                m = h["m"] + terms[c]
                fin = c == eos
                g = h["g"] + (c,)
                n = len(g) - (1 if fin else 0)
                k, r = 0.0, None
                if lam > 0:
                    k, r = ref.prefix_score(y, T, h["r"], h["g"], c, eos, blank)
                    total = (((1.0 - lam) * a + lam * k) + beta * n) + w * m
                else:
                    total = ((1.0 - lam) * a + beta * n) + w * m
                if total == NEG:
                    continue
                cands.append(dict(g=g, a=a, k=k, m=m, fin=fin, total=total, r=r))
        cands.sort(key=lambda h: -h["total"])                                # stable: ties stay in (slot, rank) order
        for p, q in zip(cands, cands[1:]):
            gap = min(gap, rel_gap(p["total"], q["total"]))
        hyps = cands[:beam]
        if not hyps:
            break
    out = [h for h in hyps if h["fin"]] + [h for h in hyps if not h["fin"]]
    return [(list(h["g"][:-1] if h["fin"] else h["g"]), h["total"], h["a"], h["k"], h["fin"], h["m"]) for h in out], gap, key_gap


# ---------------------------------------------------------------------------------------------------------------------
# the cases
def make_case_host(B, Tmax, V, seed, eos_first=0.0, eos_rest=0.0, blank=0.0, att_scale=2.0):
    """CTC log-probabilities (B, Tmax, V) and an attention table (B, Tmax + 1, V + 1, V) indexed by (utterance, step, last
    token + 1) as float32 numpy arrays, log-softmaxed on the host in float64 and rounded once: the device and the yardstick
    read the very same float32 values.  eos_first / eos_rest are added to the <eos> logit of the table's first / later
    steps, blank to the CTC blank logit."""
    rng = np.random.RandomState(seed)
    ctc = rng.randn(B, Tmax, V) * 1.5
    ctc[..., 0] += blank
    tab = rng.randn(B, Tmax + 1, V + 1, V) * att_scale
    tab[:, 0, :, V - 1] += eos_first
    tab[:, 1:, :, V - 1] += eos_rest

    def lsm(x):
        x = x - x.max(-1, keepdims=True)
        return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
    return lsm(ctc), lsm(tab)


def make_lm(tmp_path, V, order, seed):
    """A random ARPA of `order` over V - 3 words -> (path, token2char): token 0 is the blank and token V - 2 a string the
    model does not list (both <unk>), tokens 1 .. V - 3 are words, V - 1 is <eos> (reaches </s> only as the search's eos)."""
    nw = V - 3
    path = str(tmp_path / f"joint_{V}_{order}_{seed}.arpa")
    words = ngram_ref.random_arpa(path, order, nw, 40 * nw, np.random.default_rng(seed))
    return path, ["<blank>"] + words + ["oov", "<eos>"]


def prefix_lm(path, t2c):
    return PrefixLM(ngram_ref.RefLM(path), t2c)


def yardstick(y, tab, lens, plm, beam, C, lam, beta, max_steps, lm_weight, lm_prebeam):
    """Per utterance (n-best, totals' gap, keys' gap) for the table-driven scorer of make_case_host."""
    y64, V, steps = y.astype(np.float64), y.shape[2], tab.shape[1] - 1
    out = []
    for u in range(y.shape[0]):
        att = lambda g, u=u: tab[u, min(len(g), steps), (g[-1] + 1) if g else 0]     # noqa: E731
        out.append(joint_lm_search(y64[u], int(lens[u]), att, V - 1, beam, C, lam, beta, max_steps, plm, lm_weight, lm_prebeam))
    return out


# (B, Tmax, V, lens, seed of the tables)
SHAPES = {"small": (3, 7, 6, [7, 0, 1], 11), "mid": (2, 23, 12, [20, 0], 12)}
ORDERS = (2, 4)
LM_SEED = 8
# lm_weight -> (C, beta): the lighter weight with no length bonus, the heavier one with both
WEIGHTS = {0.5: (3, 0.0), 2.0: (4, 0.5)}
LAMS = (0.0, 0.3, 1.0)
BEAMS = (1, 3)
# a hypothesis that ends at the first step and then waits beside two that go on growing (as the test without an LM has it)
SURVIVOR = dict(B=2, Tmax=7, V=6, lens=[7, 6], seed=21, beam=3, C=6, lam=0.3, lm_weight=0.5, order=2,
                kw=dict(eos_first=4.0, eos_rest=-12.0, blank=3.0, att_scale=0.5))
TOTAL_GAP, KEY_GAP = 1e-8, 1e-5


def search_cases():
    """Every search of test_search_loop_against_the_yardstick: (shape, lam, beam, lm_weight, lm_prebeam, order)."""
    return list(itertools.product(SHAPES, LAMS, BEAMS, WEIGHTS, (True, False), ORDERS))
