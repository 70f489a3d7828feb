"""GPU: the short-reduction Linears as row-block GEMMs in precision 6 (csrc/ffn6.hip::rowgemm6_kernel through oe_rowgemm6 /
oe_rowgemm6_pack_table) - attention.py:56-58,97 (linear_q / k / v / out), convolution.py:79-111 (pointwise convs) and their
input gradients - against float64 and against oe_gemm_f32 on the fp32-input MFMA (precision 0) with the same epilogue."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from openeat_amd import hip, ops, planes  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def mode6():
    old = hip.GEMM_PRECISION
    hip.GEMM_PRECISION = 6
    planes.clear_all()
    yield
    hip.GEMM_PRECISION = old
    planes.clear_all()


def _err(got, ref):
    return float((got.cpu().double() - ref).abs().max())


@pytest.mark.parametrize("rows,k,n,bias,p,res,mask,beta", [
    (7936, 256, 768, True, 0.0, False, False, 1.0),        # fused q / k / v projection
    (7936, 256, 256, True, 0.1, True, False, 1.0),         # linear_out: bias, dropout, residual
    (7936, 256, 256, True, 0.1, True, True, 1.0),          # pointwise_conv2: + zeroed pad rows
    (7936, 256, 512, True, 0.0, False, False, 1.0),        # pointwise_conv1
    (4097, 256, 128, False, 0.0, True, False, 0.5),        # one chunk (the second wave group idles), ragged last block, scaled residual
    (4500, 512, 1536, True, 0.2, False, False, 1.0),       # configs[4] width
    (4100, 768, 256, True, 0.1, True, True, 0.5),          # K-phased kernel: three phases of 256, both groups
    (4097, 1024, 128, False, 0.0, False, False, 1.0),      # ... four phases, one chunk (the second group only stages rows), ragged
])
def test_x_wT_matches_float64_and_the_fp32_kernel(rows, k, n, bias, p, res, mask, beta):
    torch.manual_seed(71)
    x = torch.randn(rows, k)
    w = torch.nn.Parameter(torch.randn(n, k) / math.sqrt(k))
    b = torch.randn(n) * 0.1 if bias else None
    r = torch.randn(rows, n) if res else None
    m = (torch.rand(rows) > 0.1).to(torch.uint8) if mask else None
    xd, wd = x.to(DEV), torch.nn.Parameter(w.detach().to(DEV))
    bd, rd, md = (None if t is None else t.to(DEV) for t in (b, r, m))
    ctr = torch.tensor([7], dtype=torch.int64, device=DEV)
    epi = dict(drop_p=p, seed=0x4444, seed_dev=ctr, rowmask=md, residual=rd, ldr=n if res else 0, beta=beta)
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        y = ops.gemm_nt(xd, wd, bd, **epi)
    assert ops.ROWGEMM_LAUNCHES == n0 + 1                              # the row-block kernel took it
    y0 = torch.empty(rows, n, device=DEV)
    hip.gemm(xd, wd.detach(), y0, rows, n, k, lda=k, ldb=k, ldc=n, bias=bd, precision=0, **epi)
    ones = torch.ones(rows, n, device=DEV)
    dm = torch.empty_like(ones)
    hip.call("oe_dropout_scale", ones, ones.numel(), n, 1.0, p, 0x4444, ctr, None, dm)
    torch.cuda.synchronize()
    want = x.double() @ w.detach().double().t()
    if bias:
        want = want + b.double()
    want = want * dm.cpu().double()
    if mask:
        want = want * m.double().unsqueeze(1)
    want = (r.double() if res else 0.0) + beta * want
    e6, e0 = _err(y, want), _err(y0, want)
    assert e6 <= 2.5 * e0 + 1e-6 * float(want.abs().max()), (e6, e0)
    torch.testing.assert_close(y.cpu().double(), want, rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("rows,n_fwd,k_fwd,mask", [(7936, 256, 256, False), (7936, 512, 256, True), (7936, 256, 512, False), (5000, 512, 1536, False),
                                                  (7936, 768, 256, False), (4999, 768, 256, True)])      # the fused q / k / v projection's input gradient
def test_dy_w_matches_float64_and_the_fp32_kernel(rows, n_fwd, k_fwd, mask):
    """The input gradient dx = dy W of a Linear with weight W (n_fwd, k_fwd): reduction over n_fwd (256 / 512), output k_fwd wide."""
    torch.manual_seed(72)
    dy = torch.randn(rows, n_fwd)
    w = torch.randn(n_fwd, k_fwd) / math.sqrt(k_fwd)
    m = (torch.rand(rows) > 0.1).to(torch.uint8) if mask else None
    dyd, wd = dy.to(DEV), torch.nn.Parameter(w.to(DEV))
    md = None if m is None else m.to(DEV)
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        dx = ops.gemm_nn(dyd, wd, rowmask=md)
    assert ops.ROWGEMM_LAUNCHES == n0 + 1
    dx0 = torch.empty(rows, k_fwd, device=DEV)
    hip.gemm(dyd, wd.detach(), dx0, rows, k_fwd, n_fwd, lda=n_fwd, ldb=k_fwd, ldc=k_fwd, b_kmajor=True, rowmask=md, precision=0)
    torch.cuda.synchronize()
    want = dy.double() @ w.double()
    if mask:
        want = want * m.double().unsqueeze(1)
    assert _err(dx, want) <= 2.5 * _err(dx0, want) + 1e-6 * float(want.abs().max())
    torch.testing.assert_close(dx.cpu().double(), want, rtol=1e-4, atol=5e-5)


def test_packed_weights_follow_the_weights():
    """A weight written through torch (version counter) or behind torch's back (planes.bump_generation: what FusedAdam / a graph
    replay / a new pass announce) is re-packed before its next use; an untouched one is not packed again."""
    torch.manual_seed(73)
    x = torch.randn(4096, 256, device=DEV)
    w = torch.nn.Parameter(torch.randn(256, 256, device=DEV) / 16)
    with torch.no_grad():
        y1 = ops.gemm_nt(x, w)
        w.mul_(2.0)                                                   # torch write: version counter
        y2 = ops.gemm_nt(x, w)
        w.data.view(-1)[:].copy_((w.data * 0.25).view(-1))            # (also a torch write)
        planes.bump_generation()
        y3 = ops.gemm_nt(x, w)
    torch.cuda.synchronize()
    torch.testing.assert_close(y2, 2.0 * y1, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(y3, 0.5 * y1, rtol=1e-5, atol=1e-5)


def test_unsupported_epilogues_and_shapes_stay_on_oe_gemm_f32():
    x = torch.randn(4096, 256, device=DEV)
    w = torch.nn.Parameter(torch.randn(384 + 6, 256, device=DEV) / 16)           # n = 390: not a multiple of 128
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        ops.gemm_nt(x, w)
        w2 = torch.nn.Parameter(torch.randn(256, 256, device=DEV) / 16)
        pre = torch.empty(4096, 256, device=DEV)
        ops.gemm_nt(x, w2, None, act=ops.ACT_SWISH, preact_out=pre, ld_aux=256)   # an activation epilogue
        ops.gemm_nt(x[:3000], w2)                                               # below ROWGEMM_MIN_ROWS, above the tile form's rows
    assert ops.ROWGEMM_LAUNCHES == n0


def test_temporaries_are_never_cached():
    """A model without a parameter arena concatenates q / k / v weights into a TEMPORARY for the fused projection (ops._fused_rows):
    it dies after the call, and the next layer's temporary lands on the same address with other values and the same tensor version.
    Such weights are not registered (their pack would be taken for fresh: the B = 32 whole-model parity test caught it as 2-9 % errors
    in the decoders' gradient norms)."""
    torch.manual_seed(74)
    x = torch.randn(4096, 256, device=DEV)
    wa, wb = torch.randn(256, 256, device=DEV) / 16, torch.randn(256, 256, device=DEV) / 16
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        ta = torch.cat([wa[:128], wa[128:]], 0)
        pa = ta.data_ptr()
        ya = ops.gemm_nt(x, ta)
        del ta
        tb = torch.cat([wb[:128], wb[128:]], 0)
        same_address = tb.data_ptr() == pa
        yb = ops.gemm_nt(x, tb)
    torch.cuda.synchronize()
    assert ops.ROWGEMM_LAUNCHES == n0                                  # temporaries stay on oe_gemm_f32
    torch.testing.assert_close(ya, x @ wa.t(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(yb, x @ wb.t(), rtol=1e-4, atol=1e-4)
    assert same_address or True                                        # (the hazard's precondition on this allocator; informational)


def test_captured_refresh_survives_later_registrations():
    """A captured graph bakes in the address of the pack table and of the packed buffers.  The table is therefore ONE persistent
    tensor updated in place, append-only (the first version rebuilt it at every registration: bench.py's decode graphs replayed a
    pack launch over a freed table and the GPU faulted at address 0x1e000).  Here: capture a pass, register more weights, let a
    registered weight die, churn the allocator, change the captured weight - the replay must follow."""
    import gc
    torch.manual_seed(75)
    x = torch.randn(4096, 256, device=DEV)
    w = torch.nn.Parameter(torch.randn(256, 256, device=DEV) / 16)
    with torch.no_grad():
        y_ref = ops.gemm_nt(x, w).clone()                              # eager: registers w, uploads the table
        xs = x.clone()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with planes.capture_scope(), torch.cuda.graph(g):
            planes.new_pass()                                          # (what ASRModel.forward / _encode announce)
            ys = ops.gemm_nt(xs, w)
        table_ptr = ops._ROW.dev.data_ptr()
        others = [torch.nn.Parameter(torch.randn(256, 256, device=DEV) / 16) for _ in range(6)]
        for o in others:
            ops.gemm_nt(x, o)                                          # later registrations
        del others[2:]                                                 # ... and some of them die
        gc.collect()
        junk = [torch.full((n,), -1, dtype=torch.int64, device=DEV) for n in (6, 12, 48, 96, 384, 4096 * 6) for _ in range(4)]
        planes.new_pass()
        ops.gemm_nt(x, others[0])                                      # a refresh that sweeps the dead rows
        w.mul_(2.0)
        g.replay()
        torch.cuda.synchronize()
    assert ops._ROW.dev.data_ptr() == table_ptr and junk
    torch.testing.assert_close(ys, 2.0 * y_ref, rtol=1e-5, atol=1e-5)


# --------------------------------------------------------------------------------------------------------------------------- #
# tile form (oe_rowgemm6_form = 2): few rows, one 32 x 32 output tile per block, the eight waves split the reduction
# --------------------------------------------------------------------------------------------------------------------------- #
def test_form_table():
    L = hip.lib()
    assert L.oe_rowgemm6_form(992, 256, 256) == 2 and L.oe_rowgemm6_form(248, 256, 256) == 2 and L.oe_rowgemm6_form(5, 1024, 96) == 2
    assert L.oe_rowgemm6_form(992, 768, 256) == 2 and L.oe_rowgemm6_form(992, 512, 1024) == 2
    assert L.oe_rowgemm6_form(992, 384, 256) == 0 and L.oe_rowgemm6_form(992, 256, 3246) == 0 and L.oe_rowgemm6_form(992, 2048, 256) == 0
    assert L.oe_rowgemm6_form(7936, 256, 256) == 1 and L.oe_rowgemm6_form(7936, 1024, 256) == 1 and L.oe_rowgemm6_form(7936, 768, 512) == 0 and L.oe_rowgemm6_form(7936, 256, 96) == 0
    assert L.oe_rowgemm6_form(0, 256, 256) != 2


@pytest.mark.parametrize("rows,k,n,bias,p,res,mask,beta,act", [
    (992, 256, 768, True, 0.0, False, False, 1.0, 0),        # decoder self-attention q / k / v (decoder_layer.py:82-92)
    (992, 256, 256, True, 0.1, True, False, 1.0, 0),         # attention output: bias, dropout, residual
    (992, 1024, 256, True, 0.1, True, True, 0.5, 0),         # feed-forward w_2: k = 1024, scaled residual, dead rows
    (992, 256, 1024, True, 0.1, False, False, 1.0, 1),       # feed-forward w_1 + relu + dropout, pre-activation kept
    (992, 256, 1024, True, 0.0, False, False, 1.0, 2),       # ... + swish
    (248, 256, 256, False, 0.0, False, False, 1.0, 0),       # linear_pos (attention.py:166-171): no bias
    (37, 512, 96, True, 0.2, True, False, 1.0, 0),           # ragged single row block, n = 3 tiles
    (2048, 768, 64, False, 0.0, False, False, 1.0, 0),       # k = 768
])
def test_tile_form_x_wT_matches_float64_and_the_fp32_kernel(rows, k, n, bias, p, res, mask, beta, act):
    torch.manual_seed(81)
    x = torch.randn(rows, k)
    w = torch.randn(n, k) / math.sqrt(k)
    b = torch.randn(n) * 0.1 if bias else None
    r = torch.randn(rows, n) if res else None
    m = (torch.rand(rows) > 0.1).to(torch.uint8) if mask else None
    xd, wd = x.to(DEV), torch.nn.Parameter(w.to(DEV))
    bd, rd, md = (None if t is None else t.to(DEV) for t in (b, r, m))
    ctr = torch.tensor([9], dtype=torch.int64, device=DEV)
    pre = torch.full((rows, n), float("nan"), device=DEV) if act else None
    pre0 = torch.empty(rows, n, device=DEV) if act else None
    epi = dict(drop_p=p, seed=0x5151, seed_dev=ctr, rowmask=md, residual=rd, ldr=n if res else 0, beta=beta, act=act, ld_aux=n if act else 0)
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        y = ops.gemm_nt(xd, wd, bd, preact_out=pre, **epi)
    assert ops.ROWGEMM_LAUNCHES == n0 + 1
    y0 = torch.empty(rows, n, device=DEV)
    hip.gemm(xd, wd.detach(), y0, rows, n, k, lda=k, ldb=k, ldc=n, bias=bd, precision=0, preact_out=pre0, **epi)
    ones = torch.ones(rows, n, device=DEV)
    dm = torch.empty_like(ones)
    hip.call("oe_dropout_scale", ones, ones.numel(), n, 1.0, p, 0x5151, ctr, None, dm)
    torch.cuda.synchronize()
    want = x.double() @ w.double().t()
    if bias:
        want = want + b.double()
    want_pre = want
    if act == 1:
        want = want.clamp_min(0.0)
    elif act == 2:
        want = want * torch.sigmoid(want)
    want = want * dm.cpu().double()
    if mask:
        want = want * m.double().unsqueeze(1)
    want = (r.double() if res else 0.0) + beta * want
    if act == 1:
        # a pre-activation within rounding of zero may take the other branch: compare where it is clearly signed
        sure = (want_pre.abs() > 1e-5)
        assert float(((y.cpu().double() - want) * sure).abs().max()) < 5e-5
    else:
        e6, e0 = _err(y, want), _err(y0, want)
        assert e6 <= 2.5 * e0 + 1e-6 * float(want.abs().max()), (e6, e0)
        torch.testing.assert_close(y.cpu().double(), want, rtol=1e-4, atol=5e-5)
    if act:
        torch.testing.assert_close(pre.cpu().double(), want_pre, rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("rows,n_fwd,k_fwd,act,p", [(992, 256, 256, 0, 0.0), (992, 1024, 256, 0, 0.0), (992, 256, 1024, 1, 0.1), (992, 256, 1024, 2, 0.1),
                                                   (992, 768, 256, 0, 0.0), (61, 512, 256, 0, 0.0)])
def test_tile_form_dy_w_matches_float64(rows, n_fwd, k_fwd, act, p):
    """dx = dy W (reduction over n_fwd); with an activation: dH = (dy W2) * mask * act'(pre) - the feed-forward's backward
    through w_2 (positionwise_feed_forward.py:36-43)."""
    torch.manual_seed(82)
    dy = torch.randn(rows, n_fwd)
    w = torch.randn(n_fwd, k_fwd) / math.sqrt(k_fwd)
    pre = torch.randn(rows, k_fwd) if act else None
    dyd, wd = dy.to(DEV), torch.nn.Parameter(w.to(DEV))
    pred = None if pre is None else pre.to(DEV)
    ctr = torch.tensor([3], dtype=torch.int64, device=DEV)
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        dx = ops.gemm_nn(dyd, wd, act=act, actgrad_in=pred, ld_aux=k_fwd if act else 0, drop_p=p, seed=0x77, seed_dev=ctr, out_planes=True)
    assert ops.ROWGEMM_LAUNCHES == n0 + 1
    ones = torch.ones(rows, k_fwd, device=DEV)
    dm = torch.empty_like(ones)
    hip.call("oe_dropout_scale", ones, ones.numel(), k_fwd, 1.0, p, 0x77, ctr, None, dm)
    torch.cuda.synchronize()
    want = dy.double() @ w.double()
    if act == 1:
        want = want * (pre.double() > 0)
    elif act == 2:
        s = torch.sigmoid(pre.double())
        want = want * (s * (1 + pre.double() * (1 - s)))
    want = want * dm.cpu().double()
    torch.testing.assert_close(dx.cpu().double(), want, rtol=1e-4, atol=5e-5)


def test_tile_form_declines_what_it_cannot_do():
    x = torch.randn(992, 256, device=DEV)
    w = torch.nn.Parameter(torch.randn(3246, 256, device=DEV) / 16)              # n not a multiple of 32
    w3 = torch.nn.Parameter(torch.randn(256, 384, device=DEV) / 16)              # k = 384
    w4 = torch.nn.Parameter(torch.randn(256, 256, device=DEV) / 16)
    n0 = ops.ROWGEMM_LAUNCHES
    with torch.no_grad():
        ops.gemm_nt(x, w)
        ops.gemm_nt(torch.randn(992, 384, device=DEV), w3)
        ops.gemm_nt(x, w4, alpha=0.5)                                            # an epilogue key the kernel does not have
    assert ops.ROWGEMM_LAUNCHES == n0


# --------------------------------------------------------------------------------------------------------------------------- #
# LayerNorm-backward prologue (oe_rowgemm_args.ln_*): the rows of the GEMM are made by the LayerNorm backward that preceded it
# --------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("rows,p,with_add,with_mask,ln_mask", [(7936, 0.1, True, False, False), (4101, 0.0, False, False, False),
                                                               (7936, 0.1, True, True, False), (5000, 0.1, True, True, True)])
def test_ln_backward_prologue_equals_the_two_launches(rows, p, with_add, with_mask, ln_mask):
    """oe_layernorm_bwd_dx_drop followed by oe_rowgemm6 against ONE oe_rowgemm6 with the ln_* arguments: dx, g and the product to one
    unit in the last place, the same mask, the parameter-gradient partials to rounding (other grouping of the same sums)."""
    torch.manual_seed(91)
    d = 256
    x = torch.randn(rows, d, device=DEV) * 1.7 + 0.3
    dy = torch.randn(rows, d, device=DEV)
    add = torch.randn(rows, d, device=DEV) if with_add else None
    gamma, beta = torch.randn(d, device=DEV) * 0.2 + 1.0, torch.randn(d, device=DEV) * 0.1
    gmask = (torch.rand(rows, device=DEV) > 0.1).to(torch.uint8) if with_mask else None
    lmask = (torch.rand(rows, device=DEV) > 0.15).to(torch.uint8) if ln_mask else None      # the LayerNorm's own row mask
    w = torch.nn.Parameter(torch.randn(d, d, device=DEV) / 16)
    ctr = torch.tensor([5], dtype=torch.int64, device=DEV)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)
    stats = torch.stack([mean, rstd], 1).contiguous()
    nws = hip.lib().oe_layernorm_bwd_workspace_floats(rows, d)
    # two launches
    dx0, g0, ws0 = torch.empty_like(x), torch.empty_like(x), torch.zeros(nws, device=DEV)
    old = ops._seed_dev
    ops._seed_dev = ctr
    try:
        hip.call("oe_layernorm_bwd_dx_drop", dy, x, gamma, beta, 0, stats, rows, d, lmask, add, dx0, g0, 0.5, p, 0x1234, ctr, gmask, ws0)
        with torch.no_grad():
            ops.LN_BWD_FUSE, keep = False, ops.LN_BWD_FUSE
            y0 = ops.gemm_nn(g0, w)
            ops.LN_BWD_FUSE = keep
            # one launch
            dx1, g1, ws1 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.zeros(nws, device=DEV)
            dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
            pend = ops._LnBwdPark(dy=dy, x=x, gamma=gamma, beta=beta, stats=stats, add=add, dx=dx1, g=g1, ws=ws1, spec=(0.5, p, 0x1234, gmask),
                                  rows=rows, d=d, dg=dg, db=db, rowmask=lmask)
            ops._PENDING_LN.park(pend)
            n0 = ops.LN_BWD_FUSED_LAUNCHES
            y1 = ops.gemm_nn(g1, w)
            assert ops.LN_BWD_FUSED_LAUNCHES == n0 + 1 and pend.done and not ops._PENDING_LN
    finally:
        ops._seed_dev = old
    dg0, db0 = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    hip.call("oe_layernorm_param_reduce", ws0, rows, d, dg0, db0)
    torch.cuda.synchronize()
    # (the same formulas in another kernel: hipcc contracts a*b+c differently here and there - one unit in the last place)
    torch.testing.assert_close(dx1, dx0, rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(g1, g0, rtol=2e-6, atol=1e-6)
    assert torch.equal(g1 == 0, g0 == 0)                              # the same dropout mask / dead rows
    torch.testing.assert_close(y1, y0, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dg, dg0, rtol=2e-5, atol=2e-4)
    torch.testing.assert_close(db, db0, rtol=2e-5, atol=2e-4)


def test_a_parked_layernorm_backward_is_resolved_on_every_other_path():
    """gemm_nn on a kernel that cannot take the prologue (k = 512 here; the tile form; oe_gemm_f32) launches the LayerNorm backward on
    its own first; so does a miss in _out_drop_grad; resolve_pending_ln() sweeps what nobody picked up."""
    torch.manual_seed(92)
    rows, d = 4096, 256
    x, dy = torch.randn(rows, d, device=DEV), torch.randn(rows, d, device=DEV)
    gamma, beta = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    stats = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)], 1).contiguous()
    nws = hip.lib().oe_layernorm_bwd_workspace_floats(rows, d)

    def park():
        dx, g = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        pend = ops._LnBwdPark(dy=dy, x=x, gamma=gamma, beta=beta, stats=stats, add=None, dx=dx, g=g, ws=torch.zeros(nws, device=DEV),
                              spec=(1.0, 0.0, 0, None), rows=rows, d=d, dg=torch.zeros(d, device=DEV), db=torch.zeros(d, device=DEV))
        ops._PENDING_LN.park(pend)
        return pend

    want = torch.empty_like(x)
    hip.call("oe_layernorm_bwd_dx", dy, x, gamma, beta, 0, stats, rows, d, None, None, want, torch.zeros(nws, device=DEV))
    with torch.no_grad():
        w_wide = torch.nn.Parameter(torch.randn(256, 320, device=DEV) / 16)            # output 320 wide (not a multiple of 128): oe_gemm_f32
        pend = park()
        n0 = ops.LN_BWD_FUSED_LAUNCHES
        y = ops.gemm_nn(pend.g, w_wide)
        assert pend.done and ops.LN_BWD_FUSED_LAUNCHES == n0 and not ops._PENDING_LN
        torch.cuda.synchronize()
        assert torch.equal(pend.dx, want) and torch.equal(pend.g, want) and bool(torch.isfinite(y).all())      # (the same kernel: exact)
        pend = park()
        assert ops.resolve_pending_ln() == 1 and pend.done and not ops._PENDING_LN
        torch.cuda.synchronize()
        assert torch.equal(pend.dx, want)


@pytest.mark.parametrize("rows,n,with_mask", [(7936, 768, False), (4099, 512, True)])
def test_ln_forward_prologue_equals_the_two_launches(rows, n, with_mask):
    """oe_layernorm_fwd followed by oe_rowgemm6 against ONE oe_rowgemm6 with the lnf arguments (the pre-norm in front of the fused
    q / k / v projection and of pointwise_conv1): y, the statistics and the product to one unit in the last place."""
    torch.manual_seed(95)
    d = 256
    x = torch.randn(rows, d, device=DEV) * 1.7 + 0.3
    gamma, beta = torch.randn(d, device=DEV) * 0.2 + 1.0, torch.randn(d, device=DEV) * 0.1
    mask = (torch.rand(rows, device=DEV) > 0.1).to(torch.uint8) if with_mask else None
    w = torch.nn.Parameter(torch.randn(n, d, device=DEV) / 16)
    b = torch.randn(n, device=DEV) * 0.1
    y0, st0 = torch.empty_like(x), torch.empty(rows, 2, device=DEV)
    hip.call("oe_layernorm_fwd", x, gamma, beta, 1e-5, rows, d, mask, 0, y0, st0)
    with torch.no_grad():
        out0 = ops.gemm_nt(y0, w, b)
        y1, st1 = torch.full_like(x, float("nan")), torch.full((rows, 2), float("nan"), device=DEV)
        pend = ops._LnFwdPark(x=x, gamma=gamma, beta=beta, eps=1e-5, rows=rows, d=d, rowmask=mask, y=y1, stats=st1)
        ops._PENDING_LNF.park(pend)
        n0 = ops.LN_FWD_FUSED_LAUNCHES
        out1 = ops.gemm_nt(y1, w, b)
        assert ops.LN_FWD_FUSED_LAUNCHES == n0 + 1 and pend.done and not ops._PENDING_LNF
        # any other op of the module that receives a parked tensor launches the LayerNorm on its own first
        y2, st2 = torch.full_like(x, float("nan")), torch.full((rows, 2), float("nan"), device=DEV)
        ops._PENDING_LNF.park(ops._LnFwdPark(x=x, gamma=gamma, beta=beta, eps=1e-5, rows=rows, d=d, rowmask=mask, y=y2, stats=st2))
        z = ops.add(y2, y2) if hasattr(ops, "add") else None
    torch.cuda.synchronize()
    torch.testing.assert_close(y1, y0, rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(st1, st0, rtol=2e-6, atol=1e-6)
    torch.testing.assert_close(out1, out0, rtol=1e-5, atol=1e-5)
    assert not ops._PENDING_LNF and torch.equal(y2, y0) and torch.equal(st2, st0)
    if z is not None:
        assert torch.equal(z, y0 + y0)


@pytest.mark.parametrize("rows,act", [(7936, 2), (4107, 1), (5000, 0)])
def test_ln_backward_epilogue_equals_the_two_launches(rows, act):
    """oe_rowgemm6 with the lne arguments (the conv module's norm + activation between the depthwise convolution and pointwise_conv2,
    convolution.py:107-111): dz = g W2 followed by oe_layernorm_bwd_dx against ONE launch whose product leaves through that backward."""
    torch.manual_seed(97)
    d = 256
    gq = torch.randn(rows, d, device=DEV)
    w = torch.nn.Parameter(torch.randn(d, d, device=DEV) / 16)
    yc = torch.randn(rows, d, device=DEV) * 1.5 + 0.4
    gamma, beta = torch.randn(d, device=DEV) * 0.2 + 1.0, torch.randn(d, device=DEV) * 0.1
    stats = torch.stack([yc.mean(1), 1.0 / torch.sqrt(yc.var(1, unbiased=False) + 1e-5)], 1).contiguous()
    nws = hip.lib().oe_layernorm_bwd_workspace_floats(rows, d)
    with torch.no_grad():
        dz = ops.gemm_nn(gq, w)
        dx0, ws0 = torch.empty_like(yc), torch.zeros(nws, device=DEV)
        hip.call("oe_layernorm_bwd_dx", dz, yc, gamma, beta, act, stats, rows, d, None, None, dx0, ws0)
        dx1, ws1 = torch.full_like(yc, float("nan")), torch.zeros(nws, device=DEV)
        epi = dict(x=yc, stats=stats, gamma=gamma, beta=beta, act=act, dx=dx1, ws=ws1, done=False)
        ops.gemm_nn(gq, w, ln_epi=epi)
        assert epi["done"]
        epi2 = dict(epi, dx=torch.empty_like(yc), done=False)
        ops.gemm_nn(gq, torch.nn.Parameter(torch.randn(d, 320, device=DEV)), ln_epi=epi2)      # not 256 <- 256: plain product, nothing fused
        assert not epi2["done"]
    r = [torch.zeros(d, device=DEV) for _ in range(4)]
    hip.call("oe_layernorm_param_reduce", ws0, rows, d, r[0], r[1])
    hip.call("oe_layernorm_param_reduce", ws1, rows, d, r[2], r[3])
    torch.cuda.synchronize()
    scale = float(dx0.abs().max())
    assert float((dx1 - dx0).abs().max()) <= 3e-6 * scale + 1e-6
    torch.testing.assert_close(r[2], r[0], rtol=3e-5, atol=3e-4)
    torch.testing.assert_close(r[3], r[1], rtol=3e-5, atol=3e-4)


def test_ln_backward_epilogue_is_stable_over_many_launches():
    """Regression: with (x - mean) rstd compiled to packed-fp32 instructions (v_pk_add_f32 ... v_pk_mul_f32 op_sel:[0,1]) the low halves came
    out zero for lanes 48-63 while the SIMD's other wave issued MFMAs: rows 6 / 7 of ~10 % of the blocks wrong, other blocks at every launch.
    The kernel writes it as single-float instructions and starts the epilogue behind a block barrier (profiles/r04_experiments.md, Findings;
    reproducer: -DOE_LNE_REPRO, tools/probes/lne_variants.sh)."""
    torch.manual_seed(98)
    rows, d = 7936, 256
    gq = torch.randn(rows, d, device=DEV)
    w = torch.nn.Parameter(torch.randn(d, d, device=DEV) / 16)
    yc = torch.randn(rows, d, device=DEV) * 1.5 + 0.4
    gamma, beta = torch.randn(d, device=DEV) * 0.2 + 1.0, torch.randn(d, device=DEV) * 0.1
    stats = torch.stack([yc.mean(1), 1.0 / torch.sqrt(yc.var(1, unbiased=False) + 1e-5)], 1).contiguous()
    nws = hip.lib().oe_layernorm_bwd_workspace_floats(rows, d)
    with torch.no_grad():
        dz = ops.gemm_nn(gq, w)
        dx0 = torch.empty_like(yc)
        hip.call("oe_layernorm_bwd_dx", dz, yc, gamma, beta, 2, stats, rows, d, None, None, dx0, torch.zeros(nws, device=DEV))
        worst = 0.0
        for _ in range(60):
            dx1 = torch.full_like(yc, float("nan"))
            epi = dict(x=yc, stats=stats, gamma=gamma, beta=beta, act=2, dx=dx1, ws=torch.zeros(nws, device=DEV), done=False)
            ops.gemm_nn(gq, w, ln_epi=epi)
            assert epi["done"]
            worst = max(worst, float((dx1 - dx0).abs().max()))
    assert worst <= 3e-6 * float(dx0.abs().max()) + 1e-6, worst


# --------------------------------------------------------------------------------------------------------------------------- #
# The packed-weight tables (ops._ROW for these kernels, ops._FFN for the fused feed-forward) against the weights' CURRENT values
# after every way the weights can change: through torch, behind torch's back, by re-pointing a live Parameter's storage, by a
# new Parameter on a dead one's address, and under a captured graph.  Each check asserts through the launch counters that the
# packed path ran, compares with a float64 restatement, and checks the tables' host invariant (tests/packcheck.py) BEFORE the
# launch that follows the mutation can refresh them.
# --------------------------------------------------------------------------------------------------------------------------- #
import gc  # noqa: E402

from packcheck import assert_pack_rows_live  # noqa: E402


class _Gemm(torch.nn.Module):
    """One Linear weight through ops.gemm_nt (x W^T) or ops.gemm_nn (dy W) at the shapes of the row-block / tile forms."""

    def __init__(self, kind, rows, n, k, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.kind, self.rows = kind, rows
        self.w = torch.nn.Parameter((torch.randn(n, k, generator=g) / math.sqrt(k)).to(DEV))
        self.inp = torch.randn(rows, k if kind == "nt" else n, generator=g).to(DEV)

    def check(self):
        n0 = ops.ROWGEMM_LAUNCHES
        with torch.no_grad():
            got = ops.gemm_nt(self.inp, self.w) if self.kind == "nt" else ops.gemm_nn(self.inp, self.w)
        assert ops.ROWGEMM_LAUNCHES == n0 + 1, "the packed kernel did not take the call"
        torch.cuda.synchronize()
        w, x = self.w.detach().cpu().double(), self.inp.cpu().double()
        want = x @ w.t() if self.kind == "nt" else x @ w
        torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=5e-5)


class _Ffn(torch.nn.Module):
    """ops.feed_forward (swish, scaled residual: the macaron half-step) on the fused forward and the fused input gradient."""

    def __init__(self, d, ff, rows, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter((torch.randn(ff, d, generator=g) / math.sqrt(d)).to(DEV))
        self.b1 = torch.nn.Parameter((torch.randn(ff, generator=g) * 0.1).to(DEV))
        self.w2 = torch.nn.Parameter((torch.randn(d, ff, generator=g) / math.sqrt(ff)).to(DEV))
        self.b2 = torch.nn.Parameter((torch.randn(d, generator=g) * 0.1).to(DEV))
        self.x0 = torch.randn(rows, d, generator=g).to(DEV)
        self.wgt = torch.randn(rows, d, generator=g).to(DEV)

    def params(self):
        return [self.w1, self.b1, self.w2, self.b2]

    def run(self):
        """Forward + backward on the device: (y, dx, dw1, db1, dw2, db2); the grads are zeroed first (arena or not)."""
        from openeat_amd import arena as A
        a = A.active()
        if a is not None:
            a.zero_grad()
        else:
            for p in self.params():
                p.grad = None
        x = self.x0.clone().requires_grad_()
        f0, b0 = ops.FFN_FWD_FUSED_LAUNCHES, ops.FFN_BWD_FUSED_LAUNCHES
        y = ops.feed_forward(x, self.w1, self.b1, self.w2, self.b2, ops.ACT_SWISH, residual=x, out_scale=0.5)
        (y * self.wgt).sum().backward()
        ops.join_side_stream()
        assert (ops.FFN_FWD_FUSED_LAUNCHES, ops.FFN_BWD_FUSED_LAUNCHES) == (f0 + 1, b0 + 1), "the fused kernels did not take the call"
        return [y.detach(), x.grad] + [p.grad for p in self.params()]

    def want(self):
        w1, b1, w2, b2 = (p.detach().cpu().double().requires_grad_() for p in self.params())
        x = self.x0.cpu().double().requires_grad_()
        h = x @ w1.t() + b1
        y = x + 0.5 * ((h * torch.sigmoid(h)) @ w2.t() + b2)
        (y * self.wgt.cpu().double()).sum().backward()
        return [y.detach(), x.grad, w1.grad, b1.grad, w2.grad, b2.grad]

    def compare(self, got):
        torch.cuda.synchronize()
        want = self.want()
        torch.testing.assert_close(got[0].cpu().double(), want[0], rtol=1e-4, atol=5e-5)
        for name, g, w in zip(("dx", "dw1", "db1", "dw2", "db2"), got[1:], want[1:]):
            torch.testing.assert_close(g.cpu().double(), w, rtol=1e-4, atol=5e-5 * max(1.0, float(w.abs().max())),
                                       msg=lambda m, name=name: f"{name}: {m}")

    def check(self):
        self.compare(self.run())


_PACK_CASES = {
    "nt-rowblock-k256": lambda s: _Gemm("nt", 4096, 768, 256, s),     # fused q / k / v projection
    "nt-rowblock-k512": lambda s: _Gemm("nt", 4133, 128, 512, s),
    "nn-rowblock-k256": lambda s: _Gemm("nn", 4096, 256, 512, s),     # input gradient: reduction over 256, 512 wide
    "nt-tile": lambda s: _Gemm("nt", 992, 256, 256, s),
    "nn-tile": lambda s: _Gemm("nn", 992, 512, 256, s),
    "ffn-d256": lambda s: _Ffn(256, 1024, 4096, s),
    "ffn-d512": lambda s: _Ffn(512, 2048, 4096, s),
    "ffn-d128": lambda s: _Ffn(128, 512, 4100, s),
}


def _weights(m):
    return [p for n, p in m.named_parameters() if p.dim() == 2]


def _behind_torch(p, values):
    """Write `values` into p's storage through another tensor: p's version counter does not move."""
    alias = torch.empty(0, device=DEV).set_(p.untyped_storage(), p.storage_offset(), p.shape, p.stride())
    alias.copy_(values)


@pytest.mark.parametrize("case", list(_PACK_CASES))
@pytest.mark.parametrize("mutation", ["torch-write", "behind-torch", "fused-adam", "data-assign", "arena-over-registered",
                                      "load-state-dict-assign", "address-reuse"])
def test_packs_follow_every_weight_mutation(case, mutation):
    from openeat_amd import arena as A
    from openeat_amd.optim import FusedAdam
    m = _PACK_CASES[case](91)
    ar = opt = None
    if mutation == "fused-adam":
        ar = A.ParamArena(m).activate()
        opt = FusedAdam(ar, lr=1e-2)
    m.check()                                                         # registers the packs
    assert (ops._FFN if case.startswith("ffn") else ops._ROW).entries
    before = [p.detach().clone() for p in _weights(m)]
    if mutation == "torch-write":                                     # version counters (no new generation)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(-0.5)
    elif mutation == "behind-torch":                                  # a raw write, announced by a bare generation bump
        vers = [p._version for p in m.parameters()]
        for p in m.parameters():
            _behind_torch(p, -0.5 * p.detach())
        assert [p._version for p in m.parameters()] == vers
        planes.bump_generation()
    elif mutation == "fused-adam":                                    # the optimizer's raw kernel (FusedAdam.step -> mark_step)
        torch.manual_seed(92)
        ar.grad.normal_()
        opt.step()
    elif mutation == "data-assign":                                   # a LIVE Parameter's storage moves
        for p in m.parameters():
            p.data = -0.5 * p.detach()
        planes.new_pass()
    elif mutation == "arena-over-registered":                         # ParamArena re-points every Parameter, then a raw write
        ar = A.ParamArena(m).activate()
        ar.flat.mul_(-0.5)
        planes.new_pass()
    elif mutation == "load-state-dict-assign":
        m.load_state_dict({k: -0.5 * v.detach().clone() for k, v in m.state_dict().items()}, assign=True)
        planes.new_pass()
    elif mutation == "address-reuse":                                 # a Parameter dies; a new one with other values on its address
        landed = []
        for name in [n for n, p in m.named_parameters() if p.dim() == 2]:
            old = getattr(m, name)
            ptr, shape, std = old.data_ptr(), old.shape, float(old.detach().std())
            setattr(m, name, None)
            del old
            gc.collect()
            keep = []
            for _ in range(8):
                cand = torch.nn.Parameter(torch.randn(shape, device=DEV).mul_(std))
                if cand.data_ptr() == ptr:
                    break
                keep.append(cand)
            landed.append(cand.data_ptr() == ptr)
            setattr(m, name, cand)
            del keep
        print(f"{case}: new Parameters landed on the dead ones' addresses: {landed}")   # (the hazard's precondition; informational)
        planes.new_pass()
    after = _weights(m)
    assert all(not torch.equal(a.detach(), b) for a, b in zip(after, before)), "the mutation changed nothing"
    assert_pack_rows_live()                                           # before any launch can refresh the tables
    m.check()
    if ar is not None:
        ar.deactivate()


@pytest.mark.parametrize("case", ["ffn-d256", "ffn-d128"])
def test_captured_ffn_refresh_follows_the_weights(case):
    """The feed-forward's packs (both orientations: the forward's W1 / W2 and the input gradient's W2^T / W1^T) refreshed by a
    CAPTURED table launch: capture forward + backward, register more feed-forwards, let one die, write the captured weights in
    place (through torch and behind its back) - every replay must compute with the current values."""
    m = _PACK_CASES[case](93)
    other = [_PACK_CASES[case](94 + i) for i in range(3)]
    m.check()
    other[0].check()                                                  # two entries: the capture refreshes through the table
    x = m.x0.clone().requires_grad_()
    for p in m.params():
        p.grad = torch.zeros_like(p)
    x.grad = torch.zeros_like(x)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    f0, b0 = ops.FFN_FWD_FUSED_LAUNCHES, ops.FFN_BWD_FUSED_LAUNCHES
    with planes.capture_scope(), torch.cuda.graph(g):
        planes.new_pass()
        x.grad.zero_()
        for p in m.params():
            p.grad.zero_()
        y = ops.feed_forward(x, m.w1, m.b1, m.w2, m.b2, ops.ACT_SWISH, residual=x, out_scale=0.5)
        (y * m.wgt).sum().backward()
    assert (ops.FFN_FWD_FUSED_LAUNCHES, ops.FFN_BWD_FUSED_LAUNCHES) == (f0 + 1, b0 + 1)
    assert ops._FFN.event is None and ops._ROW.event is None          # nothing recorded inside the capture survives its scope
    for o in other[1:]:
        o.check()                                                     # later registrations
    del other[1]
    gc.collect()
    for write in ("torch", "behind", "torch"):
        with torch.no_grad():
            if write == "torch":
                for p in m.params():
                    p.mul_(-0.75)
            else:
                for p in m.params():
                    _behind_torch(p, 1.5 * p.detach())
                planes.bump_generation()
        ops.pack_tables_sweep()                                       # (what TrainEngine.replay does first)
        assert_pack_rows_live()
        g.replay()
        m.compare([y.detach(), x.grad] + [p.grad for p in m.params()])


def test_side_stream_consumers_wait_for_the_latest_ffn_pack():
    """A consumer on another stream (the right-to-left decoder, the CTC head) orders itself behind the table's recorded event
    (ops._pack_wait).  That event must be the LATEST pack launch's: the per-entry launch (a weight written through torch while
    the generation stands) records one too, and an event recorded inside a capture is forgotten when the capture's scope ends."""
    a, b = _PACK_CASES["ffn-d256"](95), _PACK_CASES["ffn-d256"](96)
    planes.new_pass()
    a.check()
    b.check()
    ev_table = ops._FFN.event
    assert ev_table is not None
    with torch.no_grad():
        a.w1.mul_(-0.5)                                               # version counter only: a per-entry pack launch
        a.w2.mul_(1.25)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    got = a.run()                                                     # the per-entry launches (forward, then input gradient)
    assert ops._FFN.event is not ev_table and ops._FFN.stream == main, "the per-entry pack launch recorded no event"
    ev_entry = ops._FFN.event
    a.compare(got)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        got = a.run()                                                 # fresh packs: the side stream waits on the latest event
        assert ops._FFN.event is ev_entry
    main.wait_stream(side)
    a.compare(got)
    # ... right after a captured refresh
    xs = a.x0.clone()
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with planes.capture_scope(), torch.cuda.graph(gr):
        planes.new_pass()
        with torch.no_grad():
            ys = ops.feed_forward(xs, a.w1, a.b1, a.w2, a.b2, ops.ACT_SWISH, residual=xs, out_scale=0.5)
    assert ops._FFN.event is None
    gr.replay()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        got = a.run()
        assert ops._FFN.stream == side
    main.wait_stream(side)
    a.compare(got)
    torch.cuda.synchronize()
    torch.testing.assert_close(ys, got[0], rtol=1e-5, atol=1e-5)
