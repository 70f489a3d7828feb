"""CPU: the yardstick of the joint CTC/attention search with n-gram LM fusion (joint_lm_search_ref.py) against the yardstick
without an LM, a greedy walk over the three-way sum and a constructed case; the gaps of every search the GPU test compares
(test_joint_lm_search_gpu.py asserts them again, here they are examined without a device); and the host-side surface of
oe_ngram_next.  No compute is launched here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ctc_prefix_score_ref as ref
import joint_lm_search_ref as R
import ngram_ref
from conftest import ROOT

NEG = -math.inf


def random_logp(rng, T, V):
    x = rng.randn(max(T, 1), V) * 1.5
    return (x - np.log(np.exp(x).sum(1, keepdims=True)))[:T] if T else np.zeros((0, V))


def table_scorer(rng, V, steps):
    x = rng.randn(steps + 1, V + 1, V) * 2.0
    tab = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)     # what a device scorer gives
    return lambda g: tab[min(len(g), steps), (g[-1] + 1) if g else 0]


@pytest.mark.parametrize("lm_prebeam", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_weight_zero_is_the_search_without_an_lm(tmp_path, lam, lm_prebeam):
    """lm_weight = 0: the n-best of ctc_prefix_score_ref.joint_search, every number exactly, in both pre-selection modes."""
    V, eos, T = 6, 5, 7
    plm = R.prefix_lm(*R.make_lm(tmp_path, V, 3, 1))
    found = 0
    for seed in range(4):
        for beam, C, beta in ((1, 2, 0.0), (3, 4, 0.25), (4, V, 0.5)):
            rng = np.random.RandomState(seed)
            y = random_logp(rng, T, V)
            att = table_scorer(rng, V, T)
            want, _ = ref.joint_search(y, T, att, eos, beam, C, lam, beta, T)
            got, _, _ = R.joint_lm_search(y, T, att, eos, beam, C, lam, beta, T, plm, 0.0, lm_prebeam)
            assert [h[:5] for h in got] == want
            found += len(got)
            for g, _, _, _, fin, m in got:                      # m is carried all the same: the sum of the terms
                seq = list(g) + ([eos] if fin else [])
                s = 0.0
                for i, c in enumerate(seq):
                    s += R.lm_term(plm, seq[:i], c, eos)
                assert m == s
    assert found > 12


@pytest.mark.parametrize("lm_prebeam", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_beam_one_is_the_greedy_walk_over_the_three_way_sum(tmp_path, lam, lm_prebeam):
    V, eos, T, C, beta, w = 6, 5, 7, 3, 0.25, 0.7
    plm = R.prefix_lm(*R.make_lm(tmp_path, V, 3, 2))
    for seed in range(4):
        rng = np.random.RandomState(10 + seed)
        y = random_logp(rng, T, V)
        att = table_scorer(rng, V, T)
        got, _, _ = R.joint_lm_search(y, T, att, eos, 1, C, lam, beta, T, plm, w, lm_prebeam)
        g, a, m, r, fin, total, k = (), 0.0, 0.0, ref.empty_state(y, T), False, 0.0, 0.0
        for _ in range(T):
            if fin:
                break
            lp = [float(x) for x in att(g)]
            term = [R.lm_term(plm, g, v, eos) for v in range(V)]
            pre = [float(np.float32(lp[v] + w * term[v])) if lm_prebeam else float(lp[v]) for v in range(V)]
            best = None
            for c in sorted(range(V), key=lambda v: (-pre[v], v))[:C]:
                kc, rc = ref.prefix_score(y, T, r, g, c, eos) if lam > 0 else (0.0, None)
                s = (1 - lam) * (a + lp[c]) + (lam * kc if lam > 0 else 0.0) + beta * (len(g) + (c != eos)) + w * (m + term[c])
                if s > NEG and (best is None or s > best[0]):
                    best = (s, c, kc, rc)
            if best is None:
                g = None
                break
            total, c, k, r = best
            a, m = a + float(lp[c]), m + term[c]
            g, fin = g + (c,), c == eos
        if g is None:
            assert got == []
            continue
        assert len(got) == 1
        toks, t_, a_, k_, f_, m_ = got[0]
        assert toks == list(g[:-1] if fin else g) and f_ == fin
        assert abs(t_ - total) < 1e-12 and abs(a_ - a) < 1e-12 and abs(k_ - k) < 1e-12 and abs(m_ - m) < 1e-12


def test_the_lm_overturns_the_decoders_first_choice(tmp_path):
    """The decoder slightly prefers token 1 at every step, the LM makes `a a` all but impossible: without the LM the best
    hypothesis repeats token 1, with it the tokens alternate.  With two candidates the LM can only reorder what the decoder
    proposes; with one candidate only the pre-selection with the LM can change anything at all."""
    path = str(tmp_path / "ab.arpa")
    ngram_ref.write_arpa(path, [[(("<s>",), -99.0, 0.0), (("</s>",), -1.0, None), (("<unk>",), -5.0, 0.0), (("a",), -0.5, 0.0),
                                 (("b",), -0.5, 0.0)],
                                [(("a", "a"), -4.0, None), (("a", "b"), -0.1, None), (("b", "a"), -0.1, None), (("b", "b"), -4.0, None)]])
    plm = R.prefix_lm(path, ["<blank>", "a", "b", "<eos>"])
    V, eos, T = 4, 3, 0
    y = np.zeros((0, V))
    lp = np.log(np.array([0.02, 0.5, 0.4, 0.08]))
    att = lambda g: lp                                                          # noqa: E731
    run = lambda C, w, pre: R.joint_lm_search(y, T, att, eos, 2, C, 0.0, 0.0, 4, plm, w, pre)[0][0][0]   # noqa: E731
    assert run(2, 0.0, True) == [1, 1, 1, 1] and run(2, 0.0, False) == [1, 1, 1, 1]
    assert run(2, 1.0, True) == [1, 2, 1, 2] and run(2, 1.0, False) == [1, 2, 1, 2]
    assert run(1, 1.0, False) == [1, 1, 1, 1]                   # the decoder's single proposal stands
    assert run(1, 1.0, True) == [1, 2, 1, 2]                    # the LM takes part in the proposal
    best = R.joint_lm_search(y, T, att, eos, 2, 2, 0.0, 0.0, 4, plm, 1.0, True)[0][0]
    a = float(lp[1] + lp[2] + lp[1] + lp[2])
    m = -0.5 + 3 * float(np.float32(-0.1))
    assert abs(best[2] - a) < 1e-12 and abs(best[5] - m) < 1e-12 and abs(best[1] - (a + m)) < 1e-12 and best[3] == 0.0


def test_the_gpu_cases_keep_their_distance(tmp_path):
    """Every search test_joint_lm_search_gpu.py compares with the yardstick, on the host: the smallest gap between neighbouring
    totals and between the C-th and (C+1)-th pre-selection key stay above what that test asserts (the seeds in
    joint_lm_search_ref.py were chosen until they did)."""
    worst_total, worst_key = math.inf, math.inf
    tables, lms = {}, {}
    for shape, lam, beam, w, pre, order in R.search_cases():
        B, Tmax, V, lens, seed = R.SHAPES[shape]
        C, beta = R.WEIGHTS[w]
        if shape not in tables:
            tables[shape] = R.make_case_host(B, Tmax, V, seed)
        if (V, order) not in lms:
            lms[V, order] = R.make_lm(tmp_path, V, order, R.LM_SEED)
        y, tab = tables[shape]
        for nb, gap, key_gap in R.yardstick(y, tab, lens, R.prefix_lm(*lms[V, order]), beam, C, lam, beta, Tmax, w, pre):
            assert gap >= R.TOTAL_GAP and key_gap >= R.KEY_GAP, (shape, lam, beam, w, pre, order, gap, key_gap)
            assert pre or key_gap == math.inf
            worst_total, worst_key = min(worst_total, gap), min(worst_key, key_gap)
    c = R.SURVIVOR
    y, tab = R.make_case_host(c["B"], c["Tmax"], c["V"], c["seed"], **c["kw"])
    plm = R.prefix_lm(*R.make_lm(tmp_path, c["V"], c["order"], R.LM_SEED))
    for pre in (True, False):
        for max_steps in (1, 2, 3, 4, 5):
            for nb, gap, key_gap in R.yardstick(y, tab, c["lens"], plm, c["beam"], c["C"], c["lam"], 0.0, max_steps, c["lm_weight"], pre):
                assert gap >= R.TOTAL_GAP and key_gap >= R.KEY_GAP, ("survivor", pre, max_steps, gap, key_gap)
                assert [h[4] for h in nb] == [True, False, False] and nb[0][0] == [], nb
                worst_total, worst_key = min(worst_total, gap), min(worst_key, key_gap)
    print(f"smallest gaps: totals {worst_total:.3g} (asserted {R.TOTAL_GAP}), pre-selection keys {worst_key:.3g} (asserted {R.KEY_GAP})")


def test_entry_point_is_declared_bound_and_validated(tmp_path):
    from openeat_amd import hip, ops
    lib = hip.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "openeat_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+oe_ngram_next\s*\(", src)
    assert "oe_ngram_next" in hip.exported_symbols() and hasattr(lib, "oe_ngram_next")
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "openeat_amd", "lib", "libopeneat_hip.so")), "oe_ngram_next")
    assert callable(ops.ngram_next)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def model(**spoil):
        kw = dict(unigrams=p, table=p, tok2word=p, capacity=4, n_words=5, max_probe=1, order=2, bos_word=0, eos_word=1, unk_word=2, V=6)
        kw.update(spoil)
        return hip.NgramModel(kw["unigrams"], kw["table"], kw["tok2word"], kw["capacity"], kw["n_words"], kw["max_probe"],
                              kw["order"], kw["bos_word"], kw["eos_word"], kw["unk_word"], kw["V"])

    def call(m=None, tokens=p, ld=3, lens=p, R=1, cand=p, C=2, eos_tok=5, out=p):
        return lib.oe_ngram_next(model() if m is None else m, tokens, ld, lens, R, cand, C, eos_tok, out, None)

    for kwargs, say in [(dict(tokens=None), b"null"), (dict(lens=None), b"null"), (dict(out=None), b"null"),
                        (dict(m=model(unigrams=None)), b"null"), (dict(m=model(table=None)), b"null"),
                        (dict(m=model(tok2word=None)), b"null"),
                        (dict(C=0), b"C must be >= 1"), (dict(C=-3), b"C must be >= 1"),
                        (dict(cand=None, C=5), b"C must equal V"), (dict(cand=None, C=7), b"C must equal V"),
                        (dict(eos_tok=6), b"eos_tok"), (dict(eos_tok=-2), b"eos_tok"), (dict(ld=-1), b"bad shape"),
                        (dict(R=-1), b"bad shape"), (dict(m=model(V=0)), b"bad shape"),
                        (dict(m=model(order=0)), b"order"), (dict(m=model(order=6)), b"order"),
                        (dict(m=model(capacity=6)), b"capacity"), (dict(m=model(max_probe=4)), b"max_probe"),
                        (dict(m=model(unk_word=5)), b"ids outside")]:
        assert call(**kwargs) != 0, kwargs
        assert say in lib.oe_last_error(), (kwargs, lib.oe_last_error())
        assert b"oe_ngram_next" in lib.oe_last_error()
    # nothing to do is not an error and launches nothing
    assert call(R=0) == 0 and call(R=0, cand=None, C=6, eos_tok=-1) == 0


def test_ops_ngram_next_refuses_host_tensors(tmp_path):
    import torch
    from openeat_amd import ops
    from openeat_amd.models.ngram_lm import NgramLM
    path, t2c = R.make_lm(tmp_path, 6, 2, 1)
    lm = NgramLM(path, t2c)
    tokens, lens = torch.zeros(2, 3, dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32)
    with pytest.raises(TypeError, match="CUDA"):
        ops.ngram_next(lm, tokens, lens)
    with pytest.raises(TypeError, match="CUDA"):
        ops.ngram_next(lm, tokens, lens, torch.zeros(2, 4, dtype=torch.int32), eos=5)
