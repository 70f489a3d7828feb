"""GPU: the kernels of csrc/optim.hip (sumsq_partial_kernel / norm_final_kernel, adam_tick_kernel / adam_kernel) and the
rel-pos kernels of csrc/elementwise.hip (relpos_prepare_rows_kernel / relpos_prepare_kernel, relpos_backward_rows_kernel /
relpos_backward_kernel) through the C ABI against the float64 yardsticks of step_f64.py, in every launch form.
* bounds: step_f64.adam_bounds(), norm_bound(), relpos_bound() - functions of the float32 restatements' caps (2 x for every
  K, 4 x for the bias-correction term C), of nothing measured here; test_step_f64_ref.py shows that the restatements meet
  them on every case used here and that every mutant misses them.  Every case is asserted; each test prints what the
  kernel needed.
* Adam: step x |g| scale x p leg (p = 0: the stored parameter is the update, judged to ulps), n around the float4 body and
  the scalar tail and over several blocks, clipped / unclipped / max_norm = 0 / no norm, device and host learning rate;
  the step count advances by exactly 1; a non-finite norm changes no bit; misaligned arenas are refused.
* norm: sizes up to two rounds of the stride loop (block 0 alone, then all 1024 blocks).
* rel-pos: the rows and the generic form of both entry points (by shape, alignment and LDS size, never by the environment
  switch), batch chunks of eight with ragged ends and short waves, several float4 columns per lane; outputs start as NaN,
  the gradient sinks start with values, the q and v thirds of the fused gradient buffer keep their bits, dk and dp repeat
  bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import step_f64 as Y  # noqa: E402
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
GUARD = 64                  # floats of canary on both sides of every output


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


class _Guarded:
    """A float32 device buffer of `n` cells filled with `fill`, between two canaries of NaN with a payload."""

    def __init__(self, n, fill=float("nan"), init=None):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
        self.buf.view(torch.int32)[:GUARD] = 0x7FC0BEEF
        self.buf.view(torch.int32)[GUARD + n:] = 0x7FC0BEEF
        self.t = self.buf[GUARD: GUARD + n]
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(_dev(init).reshape(-1))
        else:
            self.t.fill_(fill)

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:GUARD] == 0x7FC0BEEF).all()) and bool((b[GUARD + self.n:] == 0x7FC0BEEF).all())

    def host(self):
        return self.t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ Adam
def _adam_launch(key):
    """Launch oe_adam_step on adam_case(*key) -> dict(m=K, v=K, p=K at the bound's C, c=C at the bound's K, p0=K at C = 0)."""
    c = Y.adam_case(*key)
    n = c.p.size
    p, m, v = _Guarded(n, init=c.p), _Guarded(n, init=c.m), _Guarded(n, init=c.v)
    g = _dev(c.g)
    state = torch.tensor([float(c.step - 1), 0.0], device=DEV)
    norm = None if c.norm is None else torch.tensor([float(c.norm)], device=DEV)
    if c.lr_from == "dev":
        lr_dev, lr_host = torch.tensor([float(c.lr)], device=DEV), 123.0            # the host value must be ignored
    else:
        lr_dev, lr_host = None, float(c.lr)
    hip.call("oe_adam_step", p.t, g, m.t, v.t, n, lr_dev, lr_host, float(c.beta1), float(c.beta2), float(c.eps), float(c.max_norm), norm, state)
    torch.cuda.synchronize()
    assert state.tolist() == [float(c.step), 0.0], c.name
    assert p.intact() and m.intact() and v.intact(), c.name
    assert np.array_equal(g.cpu().numpy().view(np.int32), c.g.view(np.int32)), c.name
    kb, cb = Y.adam_bounds()
    ph = p.host()
    return dict(m=Y.adam_m_excess(m.host(), key), v=Y.adam_v_excess(v.host(), key), p=Y.adam_p_excess(ph, key, cb),
                c=Y.adam_p_cancel_excess(ph, key, kb["p"]), p0=Y.adam_p_excess(ph, key, 0.0))


def _adam_assert(need, what):
    kb, cb = Y.adam_bounds()
    worst = {o: max(r[o] for r in need.values()) for o in ("m", "v", "p", "c", "p0")}
    print("adam %s: kernel K of m' %.3f, v' %.3f, p' %.3f (C = %g; %.3f with C = 0); C %.3f at K = %g; bounds K %s, C %g"
          % (what, worst["m"], worst["v"], worst["p"], cb, worst["p0"], worst["c"], kb["p"], kb, cb))
    bad = {k: r for k, r in need.items() if r["m"] > kb["m"] or r["v"] > kb["v"] or r["p"] > kb["p"]}
    assert not bad, bad


@pytest.mark.parametrize("scale", Y.ADAM_SCALES)
@pytest.mark.parametrize("step", Y.ADAM_STEPS)
def test_adam_vs_float64(step, scale):
    """Both p legs, each in three of the six argument forms (all six per grid point), n = 1025: five blocks' worth of float4
    lanes in one block plus a one-element tail."""
    need = {}
    for i, form in enumerate(Y.ADAM_FORMS):
        key = (step, scale, Y.ADAM_PLEGS[i % 2], 1025, form)
        need[Y.adam_case(*key).name] = _adam_launch(key)
    _adam_assert(need, "step %d |g| %g" % (step, scale))


@pytest.mark.parametrize("n", Y.ADAM_SIZES)
def test_adam_sizes_and_argument_forms(n):
    """n < 4: the scalar tail alone; 4, 5: one vector with and without a tail; 1023 / 1025: the block's last lane; 100003: 98
    blocks.  Every argument form at every n; steps, scales and legs rotate (test_step_f64_ref.py runs the same keys)."""
    need = {}
    for i, form in enumerate(Y.ADAM_FORMS):
        key = (Y.ADAM_STEPS[(i + n) % 5], Y.ADAM_SCALES[(i + n) % 4], Y.ADAM_PLEGS[i % 2], n, form)
        need[Y.adam_case(*key).name] = _adam_launch(key)
    _adam_assert(need, "n = %d" % n)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("n", [3, 1025])
def test_adam_skips_on_a_non_finite_norm(n, bad):
    c = Y.adam_case(10, 1.0, "normal", n, Y.ADAM_FORMS[0])
    p, m, v, g = _dev(c.p), _dev(c.m), _dev(c.v), _dev(c.g)
    state = torch.tensor([9.0, 0.0], device=DEV)
    norm = torch.tensor([bad], device=DEV)
    for max_norm in (5.0, 0.0):
        hip.call("oe_adam_step", p, g, m, v, n, None, 1e-3, 0.9, 0.999, 1e-8, max_norm, norm, state)
    torch.cuda.synchronize()
    assert state.tolist() == [9.0, 0.0]
    for got, want in ((p, c.p), (m, c.m), (v, c.v)):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_misaligned_arenas_are_refused():
    """A pointer 4 bytes past a 16-byte boundary in any of p, g, m, v (and g of the norm): an error, no launch."""
    n = 64
    arrs = [torch.ones(n + 4, device=DEV) for _ in range(4)]
    state = torch.tensor([3.0, 0.0], device=DEV)
    ws = torch.empty(hip.lib().oe_grad_norm_workspace_floats(), device=DEV)
    out = torch.full((1,), -1.0, device=DEV)
    for which in range(4):
        args = [a[1: 1 + n] if i == which else a[:n] for i, a in enumerate(arrs)]
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            hip.call("oe_adam_step", *args, n, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, state)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        hip.call("oe_grad_norm", arrs[1][1: 1 + n], n, ws, out)
    torch.cuda.synchronize()
    assert state.tolist() == [3.0, 0.0] and out.item() == -1.0
    assert all(bool((a == 1.0).all()) for a in arrs)


# --------------------------------------------------------------------------------------------------------- gradient norm
@pytest.mark.parametrize("n", Y.NORM_SIZES)
def test_grad_norm_vs_float64(n):
    """One launch of 1024 blocks x 256 threads x 4 floats covers 2^20 elements: 2^20 + 1029 sends block 0 alone round the
    stride loop again (257 vectors and a tail), 3 * 2^20 + 7 every block three times."""
    ws_n = hip.lib().oe_grad_norm_workspace_floats()
    need = {}
    for kind in Y.NORM_KINDS:
        data = Y.norm_data(n, kind)
        g = _dev(data)
        ws, out = _Guarded(ws_n), _Guarded(1)
        hip.call("oe_grad_norm", g, n, ws.t, out.t)
        torch.cuda.synchronize()
        assert ws.intact() and out.intact()
        need[kind] = Y.norm_excess(out.host()[0], data)
    print("grad_norm n = %d: kernel K %s; bound %g" % (n, {k: float("%.3g" % v) for k, v in need.items()}, Y.norm_bound()))
    assert max(need.values()) <= Y.norm_bound(), need


# --------------------------------------------------------------------------------------------------------------- rel-pos
def _k_layout(k, layout, fill):
    """k (B, T, H, D) float32 placed on the device -> (the whole buffer, the view of k in it, batch stride, row stride).
    fused: the middle third of a (B, T, 3d) buffer; contiguous; shifted: the fused slice one float further, off 16-byte alignment."""
    B, T, H, D = k.shape
    d = H * D
    if layout == "contiguous":
        buf = _dev(k.reshape(B, T, d))
        return buf, buf, T * d, d
    off = 1 if layout == "shifted" else 0
    flat = torch.from_numpy(fill.astype(np.float32)).to(DEV) if fill is not None else torch.zeros(off + B * T * 3 * d + 3, device=DEV)
    assert flat.numel() == off + B * T * 3 * d + 3
    fused = flat[off: off + B * T * 3 * d].view(B, T, 3 * d)
    view = fused[:, :, d: 2 * d]
    view.copy_(_dev(k.reshape(B, T, d)))
    return flat, view, T * 3 * d, 3 * d


@pytest.mark.parametrize("layout", ["fused", "contiguous", "shifted"])
@pytest.mark.parametrize("H,D", Y.PREP_SHAPES, ids=lambda x: str(x))
def test_relpos_prepare_vs_float64(H, D, layout):
    """(4,8) (4,64) (1,4): one round of float4 columns, 2 / 16 / 1 lanes per head; (8,64) (2,256): two rounds, the second with
    the head filling a wave at D = 256; (3,12) (5,6): the generic kernel, as is every shape from the shifted slice.
    B * T = 1, 51, 10: the last block has 3, 1 and 2 waves without a row."""
    bound = Y.relpos_bound()
    need = {}
    d = H * D
    for (B, T) in Y.PREP_BT:
        c, ref = Y.relpos_case(B, T, H, D), Y.relpos_reference(B, T, H, D)
        rng = np.random.default_rng([B, T, H, D])
        fill = None if layout == "contiguous" else rng.standard_normal((1 if layout == "shifted" else 0) + B * T * 3 * d + 3)
        buf, kv, k_bs, k_rs = _k_layout(c.k, layout, fill)
        assert (kv.data_ptr() % 16 != 0) == {"contiguous": False, "fused": d % 4 != 0, "shifted": True}[layout]
        before = _bits(buf).clone()
        p, u, v = _dev(c.p.reshape(T, d)), _dev(c.u), _dev(c.v)
        kp, kb = _Guarded(B * T * d), _Guarded(B * H * T)
        hip.call("oe_relpos_prepare", kv, k_bs, k_rs, p, d, u, v, B, T, H, D, float(c.scale), kp.t, kb.t)
        torch.cuda.synchronize()
        assert kp.intact() and kb.intact() and torch.equal(_bits(buf), before)
        need[B, T] = (Y.relpos_excess(kp.host().reshape(B, T, H, D), *ref["kp"]), Y.relpos_excess(kb.host().reshape(B, H, T), *ref["keybias"]))
    print("relpos_prepare (H, D) = (%d, %d), %s k: kernel K (kp, keybias) per (B, T) %s; bound %g"
          % (H, D, layout, {k: tuple(float("%.3g" % x) for x in v) for k, v in need.items()}, bound))
    assert max(max(v) for v in need.values()) <= bound, need


def _relpos_backward(shape, misaligned_dk):
    B, T, H, D = shape
    d = H * D
    c, ref = Y.relpos_case(*shape), Y.relpos_reference(*shape)
    kbuf, kv, k_bs, k_rs = _k_layout(c.k, "fused", np.zeros(B * T * 3 * d + 3))
    dkp, dkb, p, u, v = _dev(c.dkp), _dev(c.dkb), _dev(c.p.reshape(T, d)), _dev(c.u), _dev(c.v)
    off = 1 if misaligned_dk else 0
    sentinel = np.random.default_rng([9, B, T, H, D]).standard_normal((B, T, 3 * d)).astype(np.float32)
    sentinel[:, :, d: 2 * d] = np.nan
    runs = []
    for _ in range(2):
        dqkv = _Guarded(4 + B * T * 3 * d)                       # 4 floats of slack so that the shifted view keeps its canary
        fused = dqkv.t[off: off + B * T * 3 * d].view(B, T, 3 * d)
        fused.copy_(_dev(sentinel))
        dk = fused[:, :, d: 2 * d]
        assert (dk.data_ptr() % 16 != 0) == (misaligned_dk or d % 4 != 0)
        dp, du, dv = _Guarded(T * d), _Guarded(d, init=c.du0), _Guarded(d, init=c.dv0)
        hip.call("oe_relpos_backward", dkp, dkb, kv, k_bs, k_rs, p, d, u, v, B, T, H, D, float(c.scale), dk, dp.t, d, du.t, dv.t)
        torch.cuda.synchronize()
        assert dqkv.intact() and dp.intact() and du.intact() and dv.intact(), shape
        got = fused.cpu().numpy()
        for third in (slice(0, d), slice(2 * d, 3 * d)):            # the q and v gradients: not this kernel's to touch
            assert np.array_equal(got[:, :, third].view(np.int32), sentinel[:, :, third].view(np.int32)), shape
        runs.append(dict(dk=got[:, :, d: 2 * d].reshape(B, T, H, D).copy(), dp=dp.host().reshape(T, H, D), du=du.host().reshape(H, D),
                         dv=dv.host().reshape(H, D)))
    for name in ("dk", "dp"):                                       # deterministic: no atomics, a fixed order of the batch sum
        assert np.array_equal(runs[0][name].view(np.int32), runs[1][name].view(np.int32)), (shape, name)
    assert np.array_equal(dkp.cpu().numpy(), c.dkp) and np.array_equal(kv.cpu().numpy().reshape(c.k.shape), c.k)
    return {name: max(Y.relpos_excess(r[name], *ref[name]) for r in runs) for name in ("dk", "dp", "du", "dv")}


@pytest.mark.parametrize("B", Y.BWD_BATCHES)
def test_relpos_backward_batch_chunks(B):
    """(T, H, D) = (5, 4, 64), the rows kernel with 16 lanes per head.  A wave takes ceil(B / 4) utterances in chunks of eight:
    B = 1, 3: waves without any; 4, 5: one each, the last wave short or empty; 8, 9: 2 and 3 per wave; 32: one full chunk;
    33: 9 per wave, a second chunk of one, the last wave 6; 37: 10 per wave, the last wave 7; 65: 17 per wave, three chunks."""
    need = _relpos_backward((B, 5, 4, 64), False)
    print("relpos_backward B = %d at (5, 4, 64): kernel K %s; bound %g" % (B, {k: float("%.3g" % v) for k, v in need.items()}, Y.relpos_bound()))
    assert max(need.values()) <= Y.relpos_bound(), need


@pytest.mark.parametrize("which", range(len(Y.BWD_SHAPES)), ids=["4x8", "3x12", "8x64", "4x256-lds48k", "8x256-generic", "5x6-generic", "4x64-misaligned-generic"])
def test_relpos_backward_shapes(which):
    """B in (3, 33) x T in (1, 7).  Rows form: (4,8) 8 of 64 lanes busy; (3,12) heads that do not divide a wave; (8,64) two
    float4 columns per lane; (4,256) four columns, 48 KB of LDS.  Generic form: (8,256) 96 KB would not fit; (5,6) D % 4 != 0;
    (4,64) with dk (and the whole fused gradient buffer) one float off 16-byte alignment."""
    H, D = Y.BWD_SHAPES[which]
    misaligned = which == len(Y.BWD_SHAPES) - 1
    need = {}
    for B in (3, 33):
        for T in (1, 7):
            need[B, T] = _relpos_backward((B, T, H, D), misaligned)
    worst = {name: max(r[name] for r in need.values()) for name in ("dk", "dp", "du", "dv")}
    print("relpos_backward (H, D) = (%d, %d)%s: kernel K %s; bound %g" % (H, D, " misaligned dk" if misaligned else "",
                                                                           {k: float("%.3g" % v) for k, v in worst.items()}, Y.relpos_bound()))
    assert max(worst.values()) <= Y.relpos_bound(), need
