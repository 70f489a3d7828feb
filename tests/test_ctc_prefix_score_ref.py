"""CPU: the yardstick of the joint CTC/attention search (ctc_prefix_score_ref.py) against things it does not share code with -
the prefix recursion against an enumeration of every alignment, the search against a plain beam search and a greedy walk -
and the host-side surface of oe_ctc_prefix_score.  No compute is launched here."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import ctc_prefix_score_ref as ref

NEG = -math.inf


def random_logp(rng, T, V):
    x = rng.randn(max(T, 1), V) * 1.5
    return (x - np.log(np.exp(x).sum(1, keepdims=True)))[:T] if T else np.zeros((0, V))


def close(a, b, tol=1e-9):
    if a == NEG or b == NEG:
        return a == b
    return abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize("T,V", [(1, 3), (1, 5), (4, 3), (4, 5), (6, 4)])
def test_recursion_equals_enumeration(T, V):
    """psi, the state and the <eos> score of every prefix to depth 4 - repeated tokens and prefixes longer than T included -
    against sums over all V^T alignments, to 1e-9."""
    rng = np.random.RandomState(100 * T + V)
    y = random_logp(rng, T, V)
    eos = V - 1
    tokens = list(range(1, V - 1)) if V > 2 else []
    assert tokens
    seen_long = seen_rep = 0
    for depth in range(0, 4):
        for g in itertools.product(tokens, repeat=depth):
            r = ref.state_of(y, T, g, eos)
            _, exact, state = ref.brute_force(y, T, g)
            for t in range(T):
                assert close(r[t, 0], state[t, 0]) and close(r[t, 1], state[t, 1]), (g, t, r[t], state[t])
            psi_eos, none = ref.prefix_score(y, T, r, g, eos, eos)
            assert none is None and close(psi_eos, exact), (g, psi_eos, exact)
            for c in tokens:
                psi, n = ref.prefix_score(y, T, r, g, c, eos)
                starts, _, _ = ref.brute_force(y, T, g + (c,))
                assert close(psi, starts), (g, c, psi, starts)
                assert n.shape == (T, 2)
                seen_long += len(g) + 1 > T
                seen_rep += bool(g) and g[-1] == c
                if len(g) + 1 > T:
                    assert psi == NEG
            for c in (0, -1, V, V + 3):                            # the blank and ids outside the vocabulary
                assert ref.prefix_score(y, T, r, g, c, eos) == (NEG, None)
    assert seen_rep > 0 and (seen_long > 0) == (T == 1)


def test_no_frames():
    y = np.zeros((0, 4))
    r = ref.empty_state(y, 0)
    assert r.shape == (0, 2)
    assert ref.prefix_score(y, 0, r, (), 3, eos=3) == (0.0, None)              # <eos> after the empty hypothesis
    assert ref.prefix_score(y, 0, r, (), 1, eos=3) == (NEG, None)
    assert ref.prefix_score(y, 0, r, (1,), 3, eos=3) == (NEG, None)
    assert ref.prefix_score(y, 0, r, (), 0, eos=3) == (NEG, None)
    assert ref.full_likelihood(y, 0, (), 3) == 0.0 and ref.full_likelihood(y, 0, (2,), 3) == NEG


def test_log_add_of_nothing_is_not_nan():
    assert ref.log_add(NEG, NEG) == NEG
    assert ref.log_add(NEG, -1.5) == -1.5 and ref.log_add(-1.5, NEG) == -1.5
    assert abs(ref.log_add(-1.0, -1.0) - (-1.0 + math.log(2.0))) < 1e-15


def table_scorer(rng, V, steps):
    """Attention log-probabilities that depend on (step, last token): table[step][last + 1] (row 0: no token yet)."""
    x = rng.randn(steps + 1, V + 1, V) * 2.0
    tab = x - np.log(np.exp(x).sum(-1, keepdims=True))
    return lambda g: tab[min(len(g), steps), (g[-1] + 1) if g else 0]


def plain_beam_search(att_logp, V, eos, beam, length_bonus, max_steps):
    """A plain attention beam search, written on its own: every token of every live hypothesis, stable sort, cut."""
    hyps = [((), 0.0, False)]
    for _ in range(max_steps):
        if all(f for _, _, f in hyps):
            break
        nxt = []
        for g, s, f in hyps:
            if f:
                nxt.append((g, s, f, s + length_bonus * (len(g) - 1)))
                continue
            lp = att_logp(g)
            for v in sorted(range(V), key=lambda v: (-lp[v], v)):
                h = g + (v,)
                nxt.append((h, s + float(lp[v]), v == eos, s + float(lp[v]) + length_bonus * (len(h) - (v == eos))))
        nxt.sort(key=lambda e: -e[3])
        hyps = [(g, s, f) for g, s, f, _ in nxt[:beam]]
    fin = [(g, s, f) for g, s, f in hyps if f] + [(g, s, f) for g, s, f in hyps if not f]
    return [(list(g[:-1] if f else g), s) for g, s, f in fin]


@pytest.mark.parametrize("beam,length_bonus", [(1, 0.0), (3, 0.0), (4, 0.5)])
def test_search_without_ctc_is_a_plain_beam_search(beam, length_bonus):
    V, eos, T = 6, 5, 7
    for seed in range(4):
        rng = np.random.RandomState(seed)
        y = random_logp(rng, T, V)
        att = table_scorer(rng, V, T)
        got, gap = ref.joint_search(y, T, att, eos, beam, V, 0.0, length_bonus, T)
        want = plain_beam_search(att, V, eos, beam, length_bonus, T)
        assert [g for g, *_ in got] == [g for g, _ in want]
        for (g, total, a, k, fin), (_, s) in zip(got, want):
            assert abs(a - s) < 1e-12 and k == 0.0
            assert abs(total - (a + length_bonus * len(g))) < 1e-12
        assert gap > 0


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_beam_one_is_the_greedy_walk(lam):
    """With beam = 1 the survivor of every step is the best-scoring candidate of the one hypothesis: walk it by hand."""
    V, eos, T, C = 6, 5, 7, 4
    for seed in range(4):
        rng = np.random.RandomState(10 + seed)
        y = random_logp(rng, T, V)
        att = table_scorer(rng, V, T)
        got, _ = ref.joint_search(y, T, att, eos, 1, C, lam, 0.25, T)
        g, a, r, fin, total, k = (), 0.0, ref.empty_state(y, T), False, 0.0, 0.0
        for _ in range(T):
            if fin:
                break
            lp = att(g)
            best = None
            for c in ref.top_candidates(lp, C):
                kc, rc = ref.prefix_score(y, T, r, g, c, eos) if lam > 0 else (0.0, None)
                n = len(g) + (c != eos)
                s = (1 - lam) * (a + lp[c]) + (lam * kc if lam > 0 else 0.0) + 0.25 * n
                if s > NEG and (best is None or s > best[0]):
                    best = (s, c, kc, rc)
            if best is None:
                g = None
                break
            total, c, k, r = best
            a += float(lp[c])
            g, fin = g + (c,), c == eos
        if g is None:
            assert got == []
            continue
        assert len(got) == 1
        toks, t_, a_, k_, f_ = got[0]
        assert toks == list(g[:-1] if fin else g) and f_ == fin
        assert abs(t_ - total) < 1e-12 and abs(a_ - a) < 1e-12 and abs(k_ - k) < 1e-12


def test_ctc_vetoes_an_early_eos():
    """What the mode is for: an attention scorer that prefers <eos> at once is overruled by a CTC posterior that holds tokens."""
    V, eos, T = 4, 3, 4
    y = np.log(np.full((T, V), 1e-3))
    for t, k in enumerate([1, 0, 2, 0]):
        y[t, k] = math.log(1 - 3e-3)
    lp = np.log(np.array([0.05, 0.2, 0.2, 0.55]))
    att = lambda g: lp                                                          # noqa: E731
    plain, _ = ref.joint_search(y, T, att, eos, 3, V, 0.0, 0.0, T)
    joint, _ = ref.joint_search(y, T, att, eos, 3, V, 0.5, 0.0, T)
    assert plain[0][0] == [] and joint[0][0] == [1, 2]


def test_entry_points_are_declared_bound_and_validated():
    from openeat_amd import hip
    lib = hip.lib()
    for name in ("oe_ctc_prefix_score_init", "oe_ctc_prefix_score"):
        assert name in hip.exported_symbols() and hasattr(lib, name)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def score(logp=p, B=1, Tmax=2, V=4, ldv=4, group=1, state=p, hyp_len=p, last=p, cand=p, C=2, blank=0, psi=p):
        return lib.oe_ctc_prefix_score(logp, None, B, Tmax, V, ldv, group, state, hyp_len, last, cand, C, blank, 3, psi, None, None)

    for kwargs, say in [(dict(logp=None), b"null"), (dict(state=None), b"null"), (dict(hyp_len=None), b"null"),
                        (dict(last=None), b"null"), (dict(cand=None), b"null"), (dict(psi=None), b"null"),
                        (dict(C=65), b"outside 1..64"), (dict(C=0), b"outside 1..64"), (dict(group=0), b"group"),
                        (dict(ldv=3), b"leading dimension"), (dict(blank=4), b"blank"), (dict(B=-1), b"bad shape")]:
        assert score(**kwargs) != 0, kwargs
        assert say in lib.oe_last_error(), (kwargs, lib.oe_last_error())
    assert lib.oe_ctc_prefix_score_init(None, None, 1, 2, 4, 4, 1, 0, p, None) != 0 and b"null" in lib.oe_last_error()
    assert lib.oe_ctc_prefix_score_init(p, None, 1, 2, 4, 4, 1, 0, None, None) != 0 and b"null" in lib.oe_last_error()
    assert lib.oe_ctc_prefix_score_init(p, None, 1, 2, 4, 4, 0, 0, p, None) != 0 and b"group" in lib.oe_last_error()
    # nothing to do is not an error and launches nothing
    assert score(B=0) == 0 and lib.oe_ctc_prefix_score_init(p, None, 0, 2, 4, 4, 1, 0, p, None) == 0


def test_ops_refuse_host_tensors():
    import torch
    from openeat_amd import ops
    logp = torch.zeros(1, 2, 4)
    with pytest.raises(TypeError, match="CUDA"):
        ops.ctc_prefix_score_init(logp, None)
    with pytest.raises(TypeError, match="CUDA"):
        ops.ctc_prefix_score(logp, None, torch.zeros(1, 2, 2, dtype=torch.float64), torch.zeros(1, dtype=torch.int32),
                             torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), eos=3)
