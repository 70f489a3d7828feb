"""Float64 yardsticks for the kernels that run on every training step outside the GEMMs - the gradient norm and the fused
clip + Adam update (csrc/optim.hip), rel-pos key preparation and its backward (csrc/elementwise.hip) - with their error
models, the shared data sets, float32 restatements and float32 mutants that the models must catch.  Imports nothing from
the package under test.  `python tests/step_f64.py` prints the tables below.

Adam.  adam64() is torch.optim.Adam's step on g * coef in float64; the float32 scalars (lr, betas, eps, max_norm, the norm
read from the device, the 1e-6 of the clip) enter with their float32 values, because the kernel receives floats.  With
u = lr / (1 - beta1^s) * m' / (sqrt(v') / sqrt(1 - beta2^s) + eps) the models are, per element, in units of 2^-24:

    |got - m'| <= K * 2^-24 * (beta1 |m| + (1 - beta1) |g coef|)             adam_m_excess
    |got - v'| <= K * 2^-24 * v'                                               adam_v_excess
    |got - p'| <= K * 2^-24 * (|p| + |u| (1 + (beta1 |m| + (1 - beta1) |g coef|) / |m'|))
                + C * 2^-24 * |u| (beta1^s / (1 - beta1^s) + 1/2 beta2^s / (1 - beta2^s))      adam_p_excess, adam_p_cancel_excess

(m' can cancel, and the update inherits its relative error; a relative error of beta^s, half an ulp at best, is multiplied by
beta^s / (1 - beta^s) in 1 - beta^s: 9 and 999 at step 1, where the power is exact, 4.3 and 499 at step 2, 0 at step 100000.
K and C are kept apart so that step 2 does not set the bound of step 1000: with C = 0 step 2 needs K = 30.)  In the p = 0 leg
the stored parameter is -u and the model judges it to ulps.

Clip coefficient: min(1, max_norm / (norm + 1e-6)); 1 for max_norm <= 0 or without a norm; a non-finite norm skips the step.
Its float32 rounding (two operations) is part of K: it is a relative error of g coef.

Gradient norm: sqrt(sum g^2) in float64, |got - norm| <= K * 2^-24 * norm; a zero and an infinite norm must be exact.

Rel-pos.  relpos64 / relpos_bwd64 on the upcast inputs; |got - want| <= K * 2^-24 * (sum of |terms|) per output element, the
sum of absolute terms taken in float64 next to the value (relpos_abs64, relpos_bwd_abs64): it holds for any order of
summation, the atomics over T into du / dv included, and for du / dv the sink's prefill is one more term.

K and C of the float32 restatements (adam32, torch.linalg.vector_norm, relpos32 / relpos_bwd32 with sums taken term after
term) against the yardsticks, on an x86 host (Intel Xeon, torch 2.10 with MKL, 8 threads, numpy's float32 pow and sqrt; the
caps below hold on an EPYC host with the same torch as well).  Adam:
worst of both p legs and all six argument forms at n = 1025, per step and |g| scale:

    Adam m': K             |g| 1e-09|g| 0.0001     |g| 1  |g| 1000
    step 1                     2.862     2.127     2.017     0.951
    step 2                     2.648     2.181     2.446     1.726
    step 10                    2.158     1.767     2.006     1.831
    step 1000                  2.192     1.794     2.386     1.907
    step 100000                1.896     2.180     2.330     1.709
    Adam v': K             |g| 1e-09|g| 0.0001     |g| 1  |g| 1000
    step 1                     5.768     4.038     4.444     1.896
    step 2                     4.968     3.683     3.787     2.218
    step 10                    2.576     2.334     2.223     1.805
    step 1000                  1.967     1.894     1.931     1.935
    step 100000                1.871     1.930     1.849     1.901
    Adam p': K at C = 1    |g| 1e-09|g| 0.0001     |g| 1  |g| 1000
    step 1                     0.980     0.737     0.365     0.354
    step 2                     0.987     0.921     0.943     0.933
    step 10                    0.991     0.986     0.984     0.969
    step 1000                  1.633     2.046     1.844     1.868
    step 100000                1.578     2.097     2.058     1.872
    Adam p': C at K = 3    |g| 1e-09|g| 0.0001     |g| 1  |g| 1000
    step 1                     0.000     0.000     0.000     0.000
    step 2                     0.027     0.210     0.210     0.210
    step 10                    0.000     0.023     0.011     0.022
    step 1000                  0.000     0.000     0.000     0.000
    step 100000                0.000     0.000     0.000     0.000
    K_ref = m' 2.862, v' 5.768, p' 2.097, C_ref = 0.210
    norm n            1        3        4        5     1023     1024     1025   100003  1049605  3145735
    normal        0.000    0.846    0.450    0.101    0.635    0.123    0.980    3.780  183.506 1061.650
    spike         0.000    0.000    0.000    0.000    0.000    0.000    0.000    0.008    0.088    0.264
    K_ref = 3.780 (n <= 100003)
    rel-pos (H, D)       kp  keybias       dk       dp       du       dv
    (4, 8)            1.000    1.709    1.994    1.756    2.977    1.612
    (4, 64)           1.000    1.991    1.725    2.677    3.077    2.990
    (1, 4)            0.987    1.210    1.258    1.327    0.968    1.017
    (8, 64)           1.000    1.929    1.658    2.392    3.341    2.086
    (2, 256)          1.000    1.323    1.429    2.011    2.356    2.578
    (3, 12)           1.000    1.595    2.111    1.680    1.562    1.542
    (5, 6)            0.999    3.010    1.990    1.557    2.006    2.101
    (4, 256)          1.000    1.859    1.708    2.373    2.875    2.763
    (8, 256)          1.000    2.760    1.711    2.639    2.210    2.174
    K_ref = 3.341

The caps the restatements are asserted under (test_step_f64_ref.py) and how they were chosen:
  Adam m' 3.5, v' 7, p' 3: the table's worst (2.86, 5.77, 2.10) with a fifth to a half of headroom.  They are also what a count
    of roundings gives: coef carries 2 (the sum, the quotient) and g coef one more, so (1 - beta1) g coef has 4 and m' at most
    4 + 1; the square doubles the 3 of g coef, two products and the sum bring v' to 9 in the worst case.  Nothing here but
    pow depends on the host's library: + - * / and sqrt are correctly rounded everywhere.
  Adam C 1: a correctly rounded beta^s is off by at most 2^-24 of itself, which is C = 1; the table's 0.21 is how close numpy's
    float32 pow comes on the three powers that matter (steps 2, 10, 1000); another library may use all of it.
  norm 5: torch's worst up to 100003 elements is 3.78.  Above 2^20 elements torch.linalg.vector_norm is no yardstick on this
    host (K = 184 and 1062: long float32 accumulators, six digits left) and is printed, not asserted; numpy's pairwise float32
    sum needs 2.03 there.
  rel-pos 4: the table's worst is 3.34 (du at (8, 64): 33 x 7 terms one after another).
The kernels' bounds are functions of these caps alone (adam_bounds, norm_bound, relpos_bound): 2 x the cap for every K - a
second float32 implementation of the same operations, in another order, with fused multiply-adds and a reciprocal square
root for a division; 4 x the cap for C only - the device's powf and rsqrtf are good to a few ulp where the host's pow is
close to correctly rounded, and that error is what the cancellation factor multiplies.

Measured on MI355X (tests/test_step_f64_gpu.py prints them), worst per family - adam_kernel: m' 2.65, v' 4.97 (both at step 2,
|g| 1e-9), p' 1.80 with the bound's C (step 100000, |g| 1), C 0.19 with the bound's K (step 2; 0 at every other step), K = 29.7
at step 2 if C were 0; the norm kernels 0.87 (3 * 2^20 + 7 elements, N(0,1); 0.46 at 2^20 + 1029); relpos_prepare kp 1.00,
keybias 1.38 rows form, 2.27 generic form ((5, 6)); relpos_backward rows form dk 1.55, dp 1.91, du 2.70, dv 2.48, generic form
dk 1.53, dp 2.64, du 2.85, dv 2.59 ((8, 256)).  No kernel came near a bound and none was changed.
"""
import collections
import functools
import math

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24                      # half a float32 ulp of 1: the unit of every K and C here


def up(x):
    """A scalar argument as the kernel receives it: rounded to float32, then exact in float64."""
    return float(F32(x))


def _excess(got, want, unit):
    """The smallest K with |got - want| <= K * unit in every element; inf for a non-finite `got` and where unit == 0 is missed."""
    got = np.asarray(got, dtype=np.float64)
    want, unit = np.broadcast_to(want, got.shape), np.broadcast_to(unit, got.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return math.inf
    return _worst(np.abs(got - want), unit)


def _worst(d, unit):
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(d > 0, d / unit, 0.0)          # d > 0, unit == 0 -> inf
    return float(need.max()) if need.size else 0.0


# ----------------------------------------------------------------------------------------------------------------- Adam
BETA1, BETA2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_SCALES = (1e-9, 1e-4, 1.0, 1e3)
ADAM_PLEGS = ("zero", "normal")
# (how the clip coefficient comes about, where the learning rate comes from)
ADAM_FORMS = (("clipped", "dev"), ("unclipped", "host"), ("max0", "dev"), ("nonorm", "host"), ("clipped", "host"), ("nonorm", "dev"))
ADAM_SIZES = (1, 3, 4, 5, 1023, 1025, 100003)
ADAM_MUTANTS = ("eps-in-root", "eps-scaled", "no-bc2", "step+1", "step-1", "coef-no-1e-6", "coef-m-only")
# what the float32 restatement may need per output (test_step_f64_ref.py); the module docstring says where each is from
K_ADAM_MAX, C_ADAM_MAX = dict(m=3.5, v=7.0, p=3.0), 1.0

AdamCase = collections.namedtuple("AdamCase", "p g m v step lr beta1 beta2 eps max_norm norm lr_from name")


def clip_coef64(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in float64 on the float32 values; 1 without a norm or with max_norm <= 0; None for a
    non-finite norm (the step is skipped: p, m, v and the step count keep their bits)."""
    if norm is None:
        return 1.0
    if not math.isfinite(float(norm)):
        return None
    if not max_norm > 0:
        return 1.0
    return min(1.0, up(max_norm) / (up(norm) + up(1e-6)))


def adam64(p, g, m, v, step, lr, beta1, beta2, eps, coef):
    """One Adam step (torch.optim.Adam's defaults: bias-corrected, eps outside the root and after the correction) on the
    gradient g * coef, in float64 -> (m', v', u, p' = p - u)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2, e, l = up(beta1), up(beta2), up(eps), up(lr)
    gg = g * coef
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2 = -math.expm1(step * math.log(b1)), -math.expm1(step * math.log(b2))
    u = l / bc1 * m1 / (np.sqrt(v1) / math.sqrt(bc2) + e)
    return m1, v1, u, p - u


def cancel_factor(step, beta1=BETA1, beta2=BETA2):
    """How much a relative error of beta^step grows in the update: beta1^s / (1 - beta1^s) + 1/2 * beta2^s / (1 - beta2^s)."""
    a1, a2 = math.exp(step * math.log(up(beta1))), math.exp(step * math.log(up(beta2)))
    return a1 / (1.0 - a1) + 0.5 * a2 / (1.0 - a2)


@functools.lru_cache(maxsize=None)
def _adam_ref(case_key):
    c = adam_case(*case_key)
    coef = clip_coef64(c.norm, c.max_norm)
    m1, v1, u, p1 = adam64(c.p, c.g, c.m, c.v, c.step, c.lr, c.beta1, c.beta2, c.eps, coef)
    b1 = up(c.beta1)
    am = b1 * np.abs(c.m.astype(np.float64)) + (1.0 - b1) * np.abs(c.g.astype(np.float64) * coef)
    with np.errstate(divide="ignore", invalid="ignore"):
        grow = np.where(m1 != 0, am / np.abs(m1), 0.0)
    base = U * (np.abs(c.p.astype(np.float64)) + np.abs(u) * (1.0 + grow))
    cancel = U * np.abs(u) * cancel_factor(c.step, c.beta1, c.beta2)
    return dict(m=m1, v=v1, u=u, p=p1, am=am, base=base, cancel=cancel, coef=coef)


def adam_m_excess(got, key):
    """The smallest K with |got - m'| <= K * 2^-24 * (beta1 |m| + (1 - beta1) |g coef|)."""
    r = _adam_ref(key)
    return _excess(got, r["m"], U * r["am"])


def adam_v_excess(got, key):
    """The smallest K with |got - v'| <= K * 2^-24 * v'."""
    r = _adam_ref(key)
    return _excess(got, r["v"], U * r["v"])


def adam_p_excess(got, key, C):
    """The smallest K with |got - p'| <= K * base + C * cancel (the module docstring's two terms), C given."""
    r = _adam_ref(key)
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return _worst(np.maximum(np.abs(got - r["p"]) - C * r["cancel"], 0.0), r["base"])


def adam_p_cancel_excess(got, key, K):
    """The smallest C with |got - p'| <= K * base + C * cancel, K given."""
    r = _adam_ref(key)
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return _worst(np.maximum(np.abs(got - r["p"]) - K * r["base"], 0.0), r["cancel"])


@functools.lru_cache(maxsize=None)
def adam_case(step, scale, pleg, n, form, seed=0):
    """One seeded launch: |g| ~ scale (|N(0,1)| kept above 1e-3 so that v stays a normal float32 at scale 1e-9 under the clip),
    the norm that oe_grad_norm would hand over, max_norm set from it per `form`, m and v zero at step 1 and otherwise what a
    history of such clipped gradients leaves.  Arrays are float32 and read-only."""
    clip, lr_from = form
    rng = np.random.default_rng([seed, step, ADAM_SCALES.index(scale), ADAM_PLEGS.index(pleg), n, ADAM_FORMS.index(form)])
    r = rng.standard_normal(n)
    r = np.where(r < 0, -1.0, 1.0) * np.maximum(np.abs(r), 1e-3)
    g = (scale * r).astype(F32)
    norm = F32(math.sqrt(float((g.astype(np.float64) ** 2).sum())))
    max_norm = {"clipped": F32(0.5 * float(norm)), "unclipped": F32(2.0 * float(norm) + 1e-5), "max0": F32(0.0), "nonorm": F32(5.0)}[clip]
    if clip == "nonorm":
        norm = None
    coef = clip_coef64(norm, max_norm)
    if step == 1:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    else:
        m = (coef * scale * (1.0 - BETA1 ** (step - 1)) * rng.standard_normal(n)).astype(F32)
        v = ((coef * scale) ** 2 * (1.0 - BETA2 ** (step - 1)) * (0.5 + rng.random(n))).astype(F32)
    p = np.zeros(n, F32) if pleg == "zero" else rng.standard_normal(n).astype(F32)
    for a in (p, g, m, v):
        a.setflags(write=False)
    name = "step %d, |g| %g, p %s, n %d, %s/lr %s" % (step, scale, pleg, n, clip, lr_from)
    return AdamCase(p, g, m, v, step, F32(LR), F32(BETA1), F32(BETA2), F32(EPS), max_norm, norm, lr_from, name)


def adam32(c, fault=None):
    """The kernel's formula in numpy float32 (fault None), or with one fault of ADAM_MUTANTS -> (m', v', p'):
    eps-in-root  - sqrt(v / bc2 + eps) for sqrt(v / bc2) + eps;
    eps-scaled   - (sqrt(v) + eps) / sqrt(bc2);
    no-bc2       - sqrt(v) + eps;
    step+1, -1   - both bias corrections with the neighbouring step count;
    coef-no-1e-6 - max_norm / norm;
    coef-m-only  - v takes the unclipped gradient."""
    assert fault is None or fault in ADAM_MUTANTS, fault
    one = F32(1.0)
    coef = one
    if c.norm is not None:
        if not np.isfinite(c.norm):
            return c.m.copy(), c.v.copy(), c.p.copy()
        if c.max_norm > 0:
            coef = min(one, c.max_norm / (c.norm if fault == "coef-no-1e-6" else c.norm + F32(1e-6)))
    b1, b2 = c.beta1, c.beta2
    gg = c.g * coef
    gv = c.g if fault == "coef-m-only" else gg
    m1 = b1 * c.m + (one - b1) * gg
    v1 = b2 * c.v + (one - b2) * gv * gv
    s = F32(c.step + {"step+1": 1, "step-1": -1}.get(fault, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = one - np.power(b1, s), one - np.power(b2, s)
        step_size, isb = c.lr / bc1, one / np.sqrt(bc2)
        if fault == "eps-in-root":
            den = np.sqrt(v1 * isb * isb + c.eps)
        elif fault == "eps-scaled":
            den = (np.sqrt(v1) + c.eps) * isb
        elif fault == "no-bc2":
            den = np.sqrt(v1) + c.eps
        else:
            den = np.sqrt(v1) * isb + c.eps
        p1 = c.p - step_size * m1 / den
    assert m1.dtype == v1.dtype == p1.dtype == F32
    return m1, v1, p1


def adam_ref_keys(n=1025):
    """The step x scale x p grid, every argument form at every point."""
    return [(step, scale, pleg, n, form) for step in ADAM_STEPS for scale in ADAM_SCALES for pleg in ADAM_PLEGS for form in ADAM_FORMS]


@functools.lru_cache(maxsize=None)
def adam_ref_table():
    """(step, scale) -> (K of m', K of v', K of p' with C = C_ADAM_MAX, C of p' with K = K_ADAM_MAX["p"]) of adam32, worst of
    both p legs and the six argument forms."""
    table = {}
    for key in adam_ref_keys():
        m1, v1, p1 = adam32(adam_case(*key))
        row = (adam_m_excess(m1, key), adam_v_excess(v1, key), adam_p_excess(p1, key, C_ADAM_MAX), adam_p_cancel_excess(p1, key, K_ADAM_MAX["p"]))
        table[key[:2]] = tuple(max(a, b) for a, b in zip(row, table.get(key[:2], (0.0,) * 4)))
    return table


def adam_k_ref():
    """output -> worst K of the float32 restatement over the whole grid (p' with C = C_ADAM_MAX; at step 100000, where
    beta^step is 0 and nothing can cancel, that is C = 0)."""
    rows = list(adam_ref_table().values())
    return dict(m=max(r[0] for r in rows), v=max(r[1] for r in rows), p=max(r[2] for r in rows))


def adam_c_ref():
    return max(row[3] for row in adam_ref_table().values())


def adam_bounds():
    """({output: K}, C) a kernel may need: twice the restatement's cap for K (a second float32 implementation of the same few
    operations: another order of the products, fused multiply-adds, a reciprocal square root for a division) and four times
    the cap for C (the device's powf and rsqrtf are good to a few ulp where the host's pow is close to correctly rounded, and
    that error is what the cancellation factor multiplies).  Functions of the caps alone, of nothing measured on a kernel."""
    return {o: 2.0 * k for o, k in K_ADAM_MAX.items()}, 4.0 * C_ADAM_MAX


# -------------------------------------------------------------------------------------------------------- gradient norm
NORM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 100003, (1 << 20) + 1029, 3 * (1 << 20) + 7)
NORM_KINDS = ("normal", "spike", "zeros", "inf")
NORM_SMALL = 100003                 # up to here torch's float32 sum is a yardstick (see the module docstring)
K_NORM_MAX = 5.0


@functools.lru_cache(maxsize=None)
def norm_data(n, kind):
    """float32 (n,), read-only: N(0,1); 1e-3 everywhere but the last element, 1e4; zeros; N(0,1) with the last element inf.
    The last element is in the scalar tail when n % 4, so a lost tail loses the spike."""
    rng = np.random.default_rng([7, n, NORM_KINDS.index(kind)])
    if kind == "normal":
        g = rng.standard_normal(n).astype(F32)
    elif kind == "spike":
        g = np.full(n, 1e-3, F32)
        g[n - 1] = 1e4
    elif kind == "zeros":
        g = np.zeros(n, F32)
    else:
        g = rng.standard_normal(n).astype(F32)
        g[n - 1] = np.inf
    g.setflags(write=False)
    return g


def norm64(g):
    g = np.asarray(g, dtype=np.float64)
    return math.sqrt(float((g * g).sum()))


def norm_excess(got, g):
    """The smallest K with |got - norm| <= K * 2^-24 * norm; a zero and an infinite norm must come out as such."""
    want, got = norm64(g), float(got)
    if math.isinf(want) or want == 0.0:
        return 0.0 if got == want else math.inf
    return _excess(got, want, U * want)


@functools.lru_cache(maxsize=None)
def norm_ref_table():
    """(kind, n) -> K of torch.linalg.vector_norm on the float32 data."""
    return {(kind, n): norm_excess(torch.linalg.vector_norm(torch.from_numpy(norm_data(n, kind).copy())).item(), norm_data(n, kind))
            for kind in NORM_KINDS for n in NORM_SIZES}


def norm_k_ref():
    """Worst K of the float32 reference up to NORM_SMALL elements."""
    return max(k for (_, n), k in norm_ref_table().items() if n <= NORM_SMALL)


def norm_bound():
    """The K a kernel may need, at every size: twice the cap of the float32 reference."""
    return 2.0 * K_NORM_MAX


# --------------------------------------------------------------------------------------------------------------- rel-pos
PREP_SHAPES = ((4, 8), (4, 64), (1, 4), (8, 64), (2, 256), (3, 12), (5, 6))              # (H, D): five in the rows form, two generic
PREP_BT = ((1, 1), (3, 17), (2, 5))
BWD_BATCHES = (1, 3, 4, 5, 8, 9, 32, 33, 37, 65)                                         # at (T, H, D) = (5, 4, 64)
BWD_SHAPES = ((4, 8), (3, 12), (8, 64), (4, 256), (8, 256), (5, 6), (4, 64))             # at B in (3, 33), T in (1, 7)
PREP_GRID = tuple((B, T, H, D) for (H, D) in PREP_SHAPES for (B, T) in PREP_BT)
BWD_GRID = tuple((B, 5, 4, 64) for B in BWD_BATCHES) + tuple((B, T, H, D) for (H, D) in BWD_SHAPES for B in (3, 33) for T in (1, 7))
PREP_MUTANTS = ("kb-noscale",)
BWD_MUTANTS = ("uv-swap", "chunk-dup", "chunk-drop", "du-overwrite", "head-col")
K_RELPOS_MAX = 4.0

RelposCase = collections.namedtuple("RelposCase", "k p u v scale dkp dkb du0 dv0")


@functools.lru_cache(maxsize=None)
def relpos_case(B, T, H, D, seed=0):
    """N(0,1) inputs and output gradients, float32 and read-only; du0 / dv0 are what the gradient sinks hold before the launch."""
    rng = np.random.default_rng([seed, B, T, H, D])
    f = lambda *s: rng.standard_normal(s).astype(F32)
    arrs = (f(B, T, H, D), f(T, H, D), f(H, D), f(H, D), F32(1.0 / math.sqrt(D)), f(B, T, H, D), f(B, H, T), f(H, D), f(H, D))
    for a in arrs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return RelposCase(*arrs)


def _f64(*arrs):
    return [np.asarray(a, dtype=np.float64) for a in arrs]


def _relpos64(k, p, u, v, scale):
    k, p, u, v = _f64(k, p, u, v)
    s = up(scale)
    kb = s * (np.einsum("hd,bthd->bht", u, k) + np.einsum("hd,thd->ht", v, p)[None])
    akb = s * (np.einsum("hd,bthd->bht", np.abs(u), np.abs(k)) + np.einsum("hd,thd->ht", np.abs(v), np.abs(p))[None])
    return (k + p[None], kb), (np.abs(k) + np.abs(p)[None], akb)


def relpos64(k, p, u, v, scale):
    """kp[b,t,h,:] = k + p[t,h,:]; keybias[b,h,t] = scale * (u_h . k[b,t,h] + v_h . p[t,h]) in float64 -> (kp, keybias)."""
    return _relpos64(k, p, u, v, scale)[0]


def relpos_abs64(k, p, u, v, scale):
    """The sums of the absolute values of the terms of relpos64's outputs."""
    return _relpos64(k, p, u, v, scale)[1]


def _relpos_bwd64(dkp, dkb, k, p, u, v, scale):
    dkp, dkb, k, p, u, v = _f64(dkp, dkb, k, p, u, v)
    gb = (up(scale) * dkb).transpose(0, 2, 1)[..., None]               # (B, T, H, 1)
    ab = np.abs
    val = (dkp + gb * u, (dkp + gb * v).sum(0), (gb * k).sum((0, 1)), (gb * p[None]).sum((0, 1)))
    mag = (ab(dkp) + ab(gb * u), (ab(dkp) + ab(gb * v)).sum(0), ab(gb * k).sum((0, 1)), ab(gb * p[None]).sum((0, 1)))
    return val, mag


def relpos_bwd64(dkp, dkb, k, p, u, v, scale):
    """dk = dkp + scale dkb u_h; dp = sum_b (dkp + scale dkb v_h); du = sum_bt scale dkb k; dv = sum_bt scale dkb p, in float64
    -> (dk (B,T,H,D), dp (T,H,D), du (H,D), dv (H,D)); du and dv are what the launch ADDS to its sinks."""
    return _relpos_bwd64(dkp, dkb, k, p, u, v, scale)[0]


def relpos_bwd_abs64(dkp, dkb, k, p, u, v, scale):
    return _relpos_bwd64(dkp, dkb, k, p, u, v, scale)[1]


def relpos_excess(got, want, mag):
    """The smallest K with |got - want| <= K * 2^-24 * (sum of |terms|) per element: any order of summation, the atomics included."""
    return _excess(got, want, U * mag)


def relpos32(c, fault=None):
    """The forward in numpy float32, dot products summed in index order -> (kp, keybias).  Fault kb-noscale: no `scale`."""
    assert fault is None or fault in PREP_MUTANTS, fault
    prod = c.u[None, None] * c.k + (c.v * c.p)[None]
    s = np.cumsum(prod, axis=3, dtype=F32)[..., -1].transpose(0, 2, 1)
    return c.k + c.p[None], (s if fault == "kb-noscale" else s * c.scale)


def _ragged_last(B):
    """The utterances that close a chunk of fewer than eight in relpos_backward_rows_kernel: wave w of four takes
    [w * ceil(B / 4), ...) in chunks of eight and pads the last chunk by clamping the index to its own last utterance."""
    bpw = (B + 3) // 4
    out = []
    for w in range(4):
        lo, hi = w * bpw, min(B, (w + 1) * bpw)
        if hi > lo and (hi - lo) % 8:
            out.append(hi - 1)
    return out


def relpos_bwd32(c, fault=None):
    """The backward in numpy float32, sums taken one term after another (batch inside time, as the kernels do) and added to
    du0 / dv0 -> (dk, dp, du, dv).  One fault of BWD_MUTANTS:
    uv-swap      - u in dp and v in dk;
    chunk-dup    - the utterance that closes a ragged chunk of eight counts twice in dp, du, dv (a padded slot not masked);
    chunk-drop   - that utterance is left out, and its dk stays unwritten (0 here);
    du-overwrite - du is the launch's own sum, not sink + sum;
    head-col     - the key-bias gradient's head taken from the float4 column, (j / 4) / D, not from the float column j / D."""
    assert fault is None or fault in BWD_MUTANTS, fault
    B, T, H, D = c.k.shape
    gb = (c.dkb * c.scale).transpose(0, 2, 1)                         # (B, T, H)
    if fault == "head-col":
        j = np.arange(H * D)
        gb = gb[:, :, (j // 4) // D].reshape(B, T, H, D)
    else:
        gb = np.broadcast_to(gb[..., None], (B, T, H, D))
    ud, vd = (c.v, c.u) if fault == "uv-swap" else (c.u, c.v)
    dk = c.dkp + gb * ud
    w = np.ones((B, 1, 1, 1), F32)
    if fault in ("chunk-dup", "chunk-drop"):
        last = _ragged_last(B)
        w[last] = 2.0 if fault == "chunk-dup" else 0.0
        if fault == "chunk-drop":
            dk[last] = 0.0
    seq = lambda x, ax: np.cumsum(x, axis=ax, dtype=F32).take(-1, axis=ax)
    dp = seq(w * (c.dkp + gb * vd), 0)
    tb = lambda x: (w * x).transpose(1, 0, 2, 3).reshape(T * B, H, D)
    du, dv = seq(tb(gb * c.k), 0), seq(tb(gb * c.p[None]), 0)
    du = du if fault == "du-overwrite" else c.du0 + du
    return dk, dp, du, c.dv0 + dv


RELPOS_OUTPUTS = ("kp", "keybias", "dk", "dp", "du", "dv")


@functools.lru_cache(maxsize=None)
def relpos_reference(B, T, H, D):
    """name -> (float64 value, sum of |terms|) of all six outputs on relpos_case(B, T, H, D); du / dv include the sinks' prefill."""
    c = relpos_case(B, T, H, D)
    (kp, kb), (akp, akb) = _relpos64(c.k, c.p, c.u, c.v, c.scale)
    (dk, dp, du, dv), (adk, adp, adu, adv) = _relpos_bwd64(c.dkp, c.dkb, c.k, c.p, c.u, c.v, c.scale)
    du0, dv0 = _f64(c.du0, c.dv0)
    return dict(kp=(kp, akp), keybias=(kb, akb), dk=(dk, adk), dp=(dp, adp), du=(du0 + du, np.abs(du0) + adu), dv=(dv0 + dv, np.abs(dv0) + adv))


def relpos_k(shape, fwd_fault=None, bwd_fault=None):
    """name -> K of the float32 restatement (or a mutant) on one shape; forward outputs only for a shape outside BWD_GRID's use."""
    c, ref = relpos_case(*shape), relpos_reference(*shape)
    got = dict(zip(RELPOS_OUTPUTS, relpos32(c, fwd_fault) + relpos_bwd32(c, bwd_fault)))
    return {name: relpos_excess(got[name], *ref[name]) for name in RELPOS_OUTPUTS}


@functools.lru_cache(maxsize=None)
def relpos_ref_table():
    """(H, D) -> {output: K of the float32 restatement, worst over the (B, T) of both grids}."""
    table = {}
    for shape in dict.fromkeys(PREP_GRID + BWD_GRID):
        row = table.setdefault(shape[2:], dict.fromkeys(RELPOS_OUTPUTS, 0.0))
        for name, k in relpos_k(shape).items():
            row[name] = max(row[name], k)
    return table


def relpos_k_ref():
    return max(max(row.values()) for row in relpos_ref_table().values())


def relpos_bound():
    """The K a kernel may need: twice the restatement's cap (another order of the same sums, fused multiply-adds)."""
    return 2.0 * K_RELPOS_MAX


def _print_tables():
    at = adam_ref_table()
    for col, title in enumerate(("m': K", "v': K", "p': K at C = %g" % C_ADAM_MAX, "p': C at K = %g" % K_ADAM_MAX["p"])):
        print("    %-22s" % ("Adam " + title) + "".join("%10s" % ("|g| %g" % s) for s in ADAM_SCALES))
        for step in ADAM_STEPS:
            print("    step %-17d" % step + "".join("%10.3f" % at[step, s][col] for s in ADAM_SCALES))
    print("    K_ref = %s, C_ref = %.3f" % (", ".join("%s' %.3f" % kv for kv in adam_k_ref().items()), adam_c_ref()))
    nt = norm_ref_table()
    print("    norm n    " + "".join("%9d" % n for n in NORM_SIZES))
    for kind in NORM_KINDS[:2]:
        print("    %-10s" % kind + "".join("%9.3f" % nt[kind, n] for n in NORM_SIZES))
    print("    K_ref = %.3f (n <= %d)" % (norm_k_ref(), NORM_SMALL))
    rt = relpos_ref_table()
    print("    rel-pos (H, D)" + "".join("%9s" % n for n in RELPOS_OUTPUTS))
    for hd, row in rt.items():
        print("    %-14s" % (hd,) + "".join("%9.3f" % row[n] for n in RELPOS_OUTPUTS))
    print("    K_ref = %.3f" % relpos_k_ref())


if __name__ == "__main__":
    _print_tables()
