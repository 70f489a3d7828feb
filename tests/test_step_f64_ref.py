"""CPU: pins the float64 yardsticks of step_f64.py (gradient norm, clip + Adam, rel-pos prepare / backward) and proves that
their error models have teeth.
* the float32 restatements stay inside the models on every case of the shared data sets, under the caps of step_f64.py:
  a condition on the data and the yardstick - if it fails, one of them has drifted.  The GPU test asserts every case, so
  every case has to be one the float32 arithmetic itself can meet;
* every float32 mutant, one deliberate fault each, exceeds the bound the GPU test uses (step_f64.adam_bounds, norm_bound,
  relpos_bound: functions of the caps) on at least one case of every data family it can affect; the families are listed
  at each test;
* the eps-inside-the-root mutant passes the check of test_grad_norm_and_adam_match_torch (rtol 1e-5, atol 1e-6 on p ~ 1
  after three steps) wherever no gradient element is within 1e-2 of zero after the clip, 1400 ulp off in the accumulated update."""
import math

import numpy as np
import pytest
import torch

import step_f64 as Y


# ------------------------------------------------------------------------------------------------------------------ Adam
def test_adam64_is_torch_adam():
    """The yardstick is torch.optim.Adam in float64 (after clip_grad_norm_) over three steps, to float64 round-off."""
    rng = np.random.default_rng(3)
    n = 257
    p0, g0 = rng.standard_normal(n), 3.0 * rng.standard_normal(n)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([ref], lr=Y.up(Y.LR), betas=(Y.up(Y.BETA1), Y.up(Y.BETA2)), eps=Y.up(Y.EPS))
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for it in range(3):
        g = g0 * (it + 1)
        ref.grad = torch.from_numpy(g.copy())
        tn = float(torch.nn.utils.clip_grad_norm_([ref], 5.0))
        opt.step()
        assert tn > 5.0
        m, v, u, p = Y.adam64(p, g, m, v, it + 1, Y.LR, Y.BETA1, Y.BETA2, Y.EPS, 5.0 / (tn + Y.up(1e-6)))
        np.testing.assert_allclose(p, ref.detach().numpy(), rtol=0, atol=1e-13)


def test_clip_coefficient():
    assert Y.clip_coef64(None, 5.0) == 1.0 and Y.clip_coef64(np.float32(9.0), 0.0) == 1.0 and Y.clip_coef64(np.float32(9.0), -1.0) == 1.0
    assert Y.clip_coef64(np.float32(np.inf), 5.0) is None and Y.clip_coef64(np.float32(np.nan), 5.0) is None
    assert Y.clip_coef64(np.float32(2.0), 5.0) == 1.0
    assert Y.clip_coef64(np.float32(10.0), 5.0) == 5.0 / (10.0 + float(np.float32(1e-6)))
    # the data set's forms are what their names say
    for form in Y.ADAM_FORMS:
        for scale in Y.ADAM_SCALES:
            c = Y.adam_case(10, scale, "zero", 5, form)
            coef = Y.clip_coef64(c.norm, c.max_norm)
            assert (coef < 1.0) == (form[0] == "clipped"), (form, scale, coef)
            assert (c.norm is None) == (form[0] == "nonorm")
    c = Y.adam_case(1, 1.0, "normal", 5, Y.ADAM_FORMS[0])
    assert not c.m.any() and not c.v.any() and not Y.adam_case(1, 1.0, "zero", 5, Y.ADAM_FORMS[0]).p.any()
    # a non-finite norm: the restatement returns its inputs
    bad = c._replace(norm=np.float32(np.inf))
    assert all(np.array_equal(a, b) for a, b in zip(Y.adam32(bad), (c.m, c.v, c.p)))


def test_adam_k_ref_and_c_ref():
    """The numpy float32 restatement needs K <= 3.5 (m'), 7 (v'), 3 (p') and C <= 1 on all 240 cases (5 steps x 4 scales x
    2 legs x 6 forms, n = 1025); the table is step_f64.py's docstring."""
    table = Y.adam_ref_table()
    assert len(table) == len(Y.ADAM_STEPS) * len(Y.ADAM_SCALES)
    Y._print_tables()
    k, c = Y.adam_k_ref(), Y.adam_c_ref()
    for o in "mvp":
        assert 0.25 * Y.K_ADAM_MAX[o] <= k[o] <= Y.K_ADAM_MAX[o], (o, k)     # a model four times looser than the arithmetic has drifted too
    assert c <= Y.C_ADAM_MAX
    assert c > 0.0, "no case exercises the cancellation term"
    # the cancellation term is what step 2 needs and nobody else: without it (C = 0) step 2 alone sets p's K
    worst = {step: max(Y.adam_p_excess(Y.adam32(Y.adam_case(*key))[2], key, 0.0) for key in Y.adam_ref_keys() if key[0] == step) for step in Y.ADAM_STEPS}
    print("p': K with C = 0 per step", {s: float("%.3g" % w) for s, w in worst.items()})
    assert worst[2] > 2.0 * Y.K_ADAM_MAX["p"] > 2.0 * worst[100000]
    assert Y.cancel_factor(100000) < 1e-40 and Y.cancel_factor(1) > 500.0
    assert Y.adam_bounds() == ({"m": 7.0, "v": 14.0, "p": 6.0}, 4.0)


# mutant -> (the |g| scales, the step counts) at each of which at least one case must miss the kernel's bound; None: all.
# eps-in-root / eps-scaled: where eps matters - small gradients at every step; at |g| ~ 1 only at step 1, where v = 0 lets the
#   few elements near 1e-3 show; never at |g| ~ 1e3.  eps-scaled is the true formula once bc2 = 1 (step 100000).
# no-bc2, step+-1: every scale; not step 100000, where both corrections are 1 whatever the step count.
# coef-*: the clipped forms only; the 1e-6 shows only against a norm below about 1e-2.
ADAM_FAMILIES = {
    "eps-in-root": ((1e-9, 1e-4, 1.0), None),
    "eps-scaled": ((1e-9, 1e-4, 1.0), (1, 2, 10, 1000)),
    "no-bc2": (None, (1, 2, 10, 1000)),
    "step+1": (None, (1, 2, 10, 1000)),
    "step-1": (None, (1, 2, 10, 1000)),
    "coef-no-1e-6": ((1e-9, 1e-4), None),
    "coef-m-only": (None, None),
}


def _adam_ratio(key, fault):
    kb, cb = Y.adam_bounds()
    m1, v1, p1 = Y.adam32(Y.adam_case(*key), fault)
    return max(Y.adam_m_excess(m1, key) / kb["m"], Y.adam_v_excess(v1, key) / kb["v"], Y.adam_p_excess(p1, key, cb) / kb["p"])


@pytest.mark.parametrize("fault", Y.ADAM_MUTANTS)
def test_adam_mutant_exceeds_the_gpu_bound(fault):
    assert set(ADAM_FAMILIES) == set(Y.ADAM_MUTANTS)
    scales, steps = ADAM_FAMILIES[fault]
    ratio = {key: _adam_ratio(key, fault) for key in Y.adam_ref_keys()}
    by_scale = {s: max(r for k, r in ratio.items() if k[1] == s) for s in Y.ADAM_SCALES}
    by_step = {s: max(r for k, r in ratio.items() if k[0] == s) for s in Y.ADAM_STEPS}
    print(fault, "worst excess / bound per scale", {k: float("%.3g" % v) for k, v in by_scale.items()}, "per step", {k: float("%.3g" % v) for k, v in by_step.items()})
    for s in scales or Y.ADAM_SCALES:
        assert by_scale[s] > 2.0, (fault, s, by_scale[s])
    for s in steps or Y.ADAM_STEPS:
        assert by_step[s] > 2.0, (fault, s, by_step[s])
    if fault.startswith("coef"):                        # and only where the clip acts
        assert all(r <= 1.0 for k, r in ratio.items() if k[4][0] != "clipped")
        assert all(r > 2.0 for k, r in ratio.items() if k[4][0] == "clipped" and k[1] in (scales or Y.ADAM_SCALES))


def test_unmutated_restatement_meets_the_gpu_bound_everywhere():
    """The coverage condition of the GPU test: no case of the grid is out of a float32 implementation's reach."""
    assert max(_adam_ratio(key, None) for key in Y.adam_ref_keys()) <= 0.5
    for n in Y.ADAM_SIZES:
        for i, form in enumerate(Y.ADAM_FORMS):
            key = (Y.ADAM_STEPS[(i + n) % 5], Y.ADAM_SCALES[(i + n) % 4], Y.ADAM_PLEGS[i % 2], n, form)
            assert _adam_ratio(key, None) <= 0.5, key


def _three_steps(p0, g0, max_norm, fault, dtype):
    """The loop of test_grad_norm_and_adam_match_torch: gradients g0, 2 g0, 3 g0, clipped to max_norm, from m = v = 0."""
    n = p0.size
    p, m, v = p0.astype(dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    for it in range(3):
        g = (g0 * np.float32(it + 1)).astype(np.float32)
        c = Y.AdamCase(p, g, m, v, it + 1, np.float32(Y.LR), np.float32(Y.BETA1), np.float32(Y.BETA2), np.float32(Y.EPS), np.float32(max_norm),
                       np.float32(Y.norm64(g)), "dev", "")
        if dtype is np.float64:
            m, v, _, p = Y.adam64(p, g, m, v, it + 1, c.lr, c.beta1, c.beta2, c.eps, Y.clip_coef64(c.norm, c.max_norm))
        else:
            m, v, p = Y.adam32(c, fault)
    return p


def test_eps_in_root_mutant_passes_the_old_check():
    """Why the new test exists.  test_grad_norm_and_adam_match_torch holds p ~ 1 to rtol 1e-5 / atol 1e-6 after three steps of
    lr 1e-3, that is the update to about 1e-3 of itself.  With eps inside the root the update of an element whose clipped
    gradient is g is off by eps / (2 g^2) of itself.  On that test's shape (n = 100003, |g| ~ 3, norm ~ 950 against
    max_norm 5, so clipped gradients of about 0.016) every element with |g0| >= 0.5 passes its check, up to 1e-4 of the update
    (1400 ulp over the three steps) off; only its gradients within 1e-2 of zero give the mutant away, and a data set without them - or with a
    smaller eps effect: an unclipped gradient, a norm of 10 - lets it through whole.  Against the float64 update at p = 0
    the same mutant is five orders of magnitude outside the new bound."""
    rng = np.random.default_rng(19)
    n = 100003
    r = rng.standard_normal(n)
    g0 = (3.0 * np.where(r < 0, -1.0, 1.0) * np.maximum(np.abs(r), 0.5)).astype(np.float32)
    p0 = rng.standard_normal(n).astype(np.float32)
    want = _three_steps(p0, g0, 5.0, None, np.float64)
    old = lambda got: bool((np.abs(got - want) <= 1e-6 + 1e-5 * np.abs(want)).all())
    good, bad = _three_steps(p0, g0, 5.0, None, np.float32), _three_steps(p0, g0, 5.0, "eps-in-root", np.float32)
    assert old(good) and old(bad)
    # the same three steps from p = 0, judged to ulps of the accumulated update
    z = np.zeros(n, np.float32)
    want0 = _three_steps(z, g0, 5.0, None, np.float64)
    ulps = lambda got: float((np.abs(got - want0) / (Y.U * np.abs(want0))).max())
    u_good, u_bad = ulps(_three_steps(z, g0, 5.0, None, np.float32)), ulps(_three_steps(z, g0, 5.0, "eps-in-root", np.float32))
    print("three steps from p = 0: the restatement is %.1f units of 2^-24 |u| off, the mutant %.0f" % (u_good, u_bad))
    assert u_good < 40.0 and u_bad > 1000.0


# --------------------------------------------------------------------------------------------------------- gradient norm
def test_norm_k_ref():
    """torch.linalg.vector_norm on the float32 data needs K <= 5 up to 100003 elements.  Above 2^20 it is no yardstick (its
    float32 accumulators run long: K = 184 and 1062 on the host of the table) and is printed, not asserted; the kernel's
    bound there is the one derived at the small sizes - its tree adds no level between them."""
    table = Y.norm_ref_table()
    for kind in Y.NORM_KINDS:
        print(kind, {n: float("%.3g" % table[kind, n]) for n in Y.NORM_SIZES})
    assert 0.25 <= Y.norm_k_ref() <= Y.K_NORM_MAX == 5.0
    assert Y.norm_bound() == 10.0
    for n in Y.NORM_SIZES:
        assert table["zeros", n] == 0.0 and table["inf", n] == 0.0
        assert Y.norm_excess(np.float32(np.sqrt(np.sum(Y.norm_data(n, "normal") ** 2, dtype=np.float32))), Y.norm_data(n, "normal")) <= Y.K_NORM_MAX
    assert Y.norm_excess(1.0, np.zeros(3, np.float32)) == math.inf and Y.norm_excess(3.0, Y.norm_data(5, "inf")) == math.inf
    assert Y.norm_excess(np.float32(np.nan), Y.norm_data(5, "normal")) == math.inf


@pytest.mark.parametrize("n", Y.NORM_SIZES)
def test_norm_faults_exceed_the_gpu_bound(n):
    """A lost scalar tail loses the spike; at the two sizes above one round of the kernel's stride loop (2^20 floats), a sum
    that stops after the first round or counts it twice misses the bound on N(0,1)."""
    bound = Y.norm_bound()
    spike = Y.norm_data(n, "spike")
    if n % 4:
        assert Y.norm_excess(np.float32(Y.norm64(spike[: n - n % 4])), spike) > 100.0 * bound
    g = Y.norm_data(n, "normal")
    if n > 1 << 20:
        once = g[: 1 << 20].astype(np.float64)
        assert Y.norm_excess(np.float32(Y.norm64(once)), g) > 100.0 * bound
        assert Y.norm_excess(np.float32(math.sqrt(Y.norm64(g) ** 2 + Y.norm64(once[:1024]) ** 2)), g) > 100.0 * bound


# --------------------------------------------------------------------------------------------------------------- rel-pos
def test_relpos64_is_autograd():
    """The forward yardstick is the einsum definition; the backward one is its float64 autograd."""
    c = Y.relpos_case(3, 7, 3, 12)
    k, p, u, v = (torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_() for a in (c.k, c.p, c.u, c.v))
    kp = k + p[None]
    kb = Y.up(c.scale) * (torch.einsum("hd,bthd->bht", u, k) + torch.einsum("hd,thd->ht", v, p)[None])
    got_kp, got_kb = Y.relpos64(c.k, c.p, c.u, c.v, c.scale)
    np.testing.assert_allclose(got_kp, kp.detach().numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got_kb, kb.detach().numpy(), rtol=0, atol=1e-13)
    ((kp * torch.from_numpy(c.dkp.astype(np.float64))).sum() + (kb * torch.from_numpy(c.dkb.astype(np.float64))).sum()).backward()
    for got, want in zip(Y.relpos_bwd64(c.dkp, c.dkb, c.k, c.p, c.u, c.v, c.scale), (k.grad, p.grad, u.grad, v.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)
    for val, mag in zip(Y.relpos_bwd64(c.dkp, c.dkb, c.k, c.p, c.u, c.v, c.scale), Y.relpos_bwd_abs64(c.dkp, c.dkb, c.k, c.p, c.u, c.v, c.scale)):
        assert val.shape == mag.shape and bool((np.abs(val) <= mag * (1 + 1e-12)).all())


def test_relpos_grids():
    assert len(Y.PREP_GRID) == 21 and len(Y.BWD_GRID) == 10 + 28
    # the shapes reach both forms of both entry points: rows needs D / 4 a power of two (prepare), D % 4 == 0 and 48 H D bytes of LDS
    # within 64 KB (backward)
    prep_rows = lambda H, D: D % 4 == 0 and (D // 4) & (D // 4 - 1) == 0 and D // 4 <= 64
    bwd_rows = lambda H, D: D % 4 == 0 and 48 * H * D <= 64 * 1024
    assert [prep_rows(*s) for s in Y.PREP_SHAPES] == [True] * 5 + [False] * 2
    assert [bwd_rows(*s) for s in Y.BWD_SHAPES] == [True, True, True, True, False, False, True]
    assert 48 * 4 * 256 == 48 * 1024
    # ragged chunks: every batch size of the grid but 32 has a wave whose last chunk of eight is short
    assert [bool(Y._ragged_last(B)) for B in Y.BWD_BATCHES] == [True] * 6 + [False] + [True] * 3
    assert Y._ragged_last(37) == [9, 19, 29, 36] and Y._ragged_last(33) == [8, 17, 26, 32] and Y._ragged_last(5) == [1, 3, 4]


def test_relpos_k_ref():
    """The numpy float32 restatement (sums taken term after term) needs K <= 4 on every output and shape of both grids."""
    table = Y.relpos_ref_table()
    assert set(table) == set(Y.PREP_SHAPES) | set(Y.BWD_SHAPES)
    for hd, row in table.items():
        print(hd, {k: float("%.3g" % v) for k, v in row.items()})
    assert 1.0 <= Y.relpos_k_ref() <= Y.K_RELPOS_MAX == 4.0
    assert Y.relpos_bound() == 8.0


def test_relpos_prepare_mutant_exceeds_the_gpu_bound():
    """keybias without `scale`: every shape (scale = 1 / sqrt(D) is never 1)."""
    for shape in Y.PREP_GRID:
        k = Y.relpos_k(shape, fwd_fault="kb-noscale")
        assert k["keybias"] > 100.0 * Y.relpos_bound() and k["kp"] <= Y.K_RELPOS_MAX, shape


# mutant -> the outputs that must miss the bound, on every shape of BWD_GRID the mutant can affect:
# chunk-dup / chunk-drop: every batch size with a ragged chunk (all of the grid's but 32: four full chunks of eight);
# du-overwrite: every shape, because the sinks are prefilled; head-col: every shape (H > 1 throughout).
BWD_FAMILIES = {"uv-swap": ("dk", "dp"), "chunk-dup": ("dp", "du", "dv"), "chunk-drop": ("dk", "dp", "du", "dv"), "du-overwrite": ("du",),
                "head-col": ("dk", "dp", "du", "dv")}


@pytest.mark.parametrize("fault", Y.BWD_MUTANTS)
def test_relpos_backward_mutant_exceeds_the_gpu_bound(fault):
    bound = Y.relpos_bound()
    for shape in Y.BWD_GRID:
        k = Y.relpos_k(shape, bwd_fault=fault)
        hidden = fault.startswith("chunk") and not Y._ragged_last(shape[0])
        for name in ("dk", "dp", "du", "dv"):
            if name in BWD_FAMILIES[fault] and not hidden:
                assert k[name] > 100.0 * bound, (fault, shape, name, k[name])
            else:
                assert k[name] <= Y.K_RELPOS_MAX, (fault, shape, name, k[name])
