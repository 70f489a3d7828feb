"""GPU: oe_ctc_nbest_score / oe_ctc_nbest_grad (raw C ABI) and ops.ctc_nbest_logp against the float64 yardstick
tests/ctc_nbest_ref.py.  Tolerances are those of test_ctc_vs_oracle: logp rtol 1e-4 / atol 1e-3; dlogits rtol 2e-3 / atol
2e-5 * max(1, sum of |g| over the utterance's feasible rows) - each hypothesis contributes at most the loss's error times its
weight.  The padding behind a hypothesis' length holds VALID token ids that would change the answer if read; outputs are
prefilled with a sentinel."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_nbest_ref as ref  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402

DEV = "cuda"
SENT = -777.0


class Case:
    def __init__(self, B, group, T, V, ldv, Lmax, hlens, hyps, lens, seed):
        self.B, self.group, self.T, self.V, self.ldv, self.Lmax = B, group, T, V, ldv, Lmax
        self.R = B * group
        gen = torch.Generator().manual_seed(seed)
        self.logits = torch.randn(B, T, V, generator=gen) * 2.0
        self.hlens = torch.tensor(hlens, dtype=torch.int32)
        self.hyps = hyps.to(torch.int32).contiguous()              # (R, hyp_ld >= Lmax)
        self.lens = torch.as_tensor(lens, dtype=torch.int32)
        assert self.hyps.shape[0] == self.R and self.hyps.shape[1] >= Lmax and self.lens.shape == (self.R,)
        self.bad = ref.infeasible_rows(hlens, self.hyps[:, :Lmax], self.lens, group, V, Lmax, T)
        self.g = torch.rand(self.R, generator=gen) * 2 - 1
        self.g[self.bad] = float("nan")                            # g of an infeasible row reaches nothing
        self.want_logp, self.want_dx = ref.nbest_grad(self.logits.double(), hlens, self.hyps[:, :Lmax], self.lens, group,
                                                      torch.nan_to_num(self.g).view(B, group))


def _device_run(c, hyps=None, lens=None, g=None, with_saved=True, grad=True):
    """-> logp (R) and dlogits (B, T, ldv) on the CPU (dlogits None without grad)."""
    hyps = c.hyps if hyps is None else hyps
    lens = c.lens if lens is None else lens
    g = c.g if g is None else g
    buf = torch.full((c.B, c.T, c.ldv), 0.25, device=DEV)          # the padding columns hold an ordinary number
    buf[..., : c.V] = c.logits.to(DEV)
    dl = torch.full((c.B, c.T, c.ldv), SENT, device=DEV)
    logp = torch.full((c.R,), SENT, device=DEV)
    lib = hip.lib()
    ws = torch.empty(lib.oe_ctc_nbest_workspace_bytes(c.B, c.T, c.group, c.Lmax), dtype=torch.uint8, device=DEV)
    saved = torch.empty(lib.oe_ctc_nbest_saved_bytes(c.B, c.T, c.group, c.Lmax), dtype=torch.uint8, device=DEV) if with_saved else None
    args = (buf, c.ldv, c.B, c.T, c.V, c.hlens.to(DEV), hyps.to(DEV), hyps.shape[1], lens.to(DEV), c.group, c.Lmax)
    hip.call("oe_ctc_nbest_score", *args, logp, saved, ws)
    if grad:
        assert with_saved
        hip.call("oe_ctc_nbest_grad", *args, logp, g.to(DEV), saved, dl, None)
    torch.cuda.synchronize()
    return logp.cpu(), (dl.cpu() if grad else None)


def _check(c):
    logp, dl = _device_run(c)
    want = c.want_logp.view(-1)
    # -inf exactly where the rule says, and only there
    assert torch.equal(torch.isinf(logp) & (logp < 0), c.bad), (logp, c.bad)
    fin = ~c.bad
    err = (logp[fin].double() - want[fin]).abs()
    tol = 1e-3 + 1e-4 * want[fin].abs()
    print(f"logp: max err {float(err.max()) if fin.any() else 0.0:.3g} (largest |logp| {float(want[fin].abs().max()) if fin.any() else 0.0:.4g})")
    assert (err <= tol).all(), (logp, want)
    # the gradient
    got = dl[..., : c.V].double()
    gsum = torch.nan_to_num(c.g).abs().view(c.B, c.group).sum(1).clamp(min=1.0).double()
    tol = 2e-5 * gsum.view(c.B, 1, 1) + 2e-3 * c.want_dx.abs()
    derr = (got - c.want_dx).abs()
    print(f"dlogits: max err {float(derr.max()):.3g}, max |ref| {float(c.want_dx.abs().max()):.3g}, worst err / tol {float((derr / tol).max()):.3g}")
    assert torch.isfinite(got).all() and (derr <= tol).all()
    for b in range(c.B):
        Tb = min(max(int(c.hlens[b]), 0), c.T)
        assert (dl[b, Tb:, : c.V] == 0).all()                      # padded frames: exact zeros
    assert (dl[..., c.V:] == SENT).all()                           # columns >= V are not written
    # bit-identical: with and without `saved`, from run to run, under a permutation of the slots
    logp_ns, _ = _device_run(c, with_saved=False, grad=False)
    assert torch.equal(logp_ns.view(torch.int32), logp.view(torch.int32))
    logp2, dl2 = _device_run(c)
    assert torch.equal(logp2.view(torch.int32), logp.view(torch.int32)) and torch.equal(dl2.view(torch.int32), dl.view(torch.int32))
    if c.group > 1:
        perm = torch.arange(c.R).view(c.B, c.group).roll(1, 1).flip(1).reshape(-1)
        logp_p, _ = _device_run(c, hyps=c.hyps[perm].contiguous(), lens=c.lens[perm].contiguous(), with_saved=False, grad=False)
        assert torch.equal(logp_p.view(torch.int32), logp[perm].view(torch.int32))
    return logp, dl


def _pad_fill(R, width, V):
    """Valid token ids everywhere: what lies behind a length would change the answer if it were read."""
    return (torch.arange(R).view(R, 1) * 3 + torch.arange(width).view(1, width) * 5) % (V - 1) + 1


def _random_case(B, group, T, V, ldv, Lmax, hlens, seed, lo, hi, missing=True, fixed_lens=None):
    """Near-duplicate lists: every slot is its utterance's base sequence with one or two positions changed and a repeat forced."""
    gen = torch.Generator().manual_seed(seed)
    R = B * group
    hyps = _pad_fill(R, Lmax + 1, V)                               # hyp_ld = Lmax + 1
    lens = torch.zeros(R, dtype=torch.int32)
    for b in range(B):
        base = torch.randint(1, V, (Lmax,), generator=gen)
        for n in range(group):
            r = b * group + n
            L = int(torch.randint(lo, hi + 1, (1,), generator=gen)) if fixed_lens is None else fixed_lens[r]
            row = base.clone()
            for _ in range(1 + n % 2):
                if Lmax:
                    row[int(torch.randint(0, Lmax, (1,), generator=gen))] = int(torch.randint(1, V, (1,), generator=gen))
            if L >= 2 and n % 3 == 1:
                k = int(torch.randint(0, L - 1, (1,), generator=gen))
                row[k + 1] = row[k]                                # an adjacent repeat
            hyps[r, :L] = row[:L]
            lens[r] = L
        if missing and group > 2:
            lens[b * group + group - 2] = -1
    return Case(B, group, T, V, ldv, Lmax, hlens, hyps, lens, seed + 1000)


@pytest.mark.parametrize("hlens", [(12, 3, 1), (9, 0, 3)])
def test_hand_written_lists(hlens):
    """(B, group, T, V, ldv, Lmax) = (3, 4, 12, 7, 8, 6): a near-duplicate pair, a repeat, a missing slot, the empty hypothesis,
    three equal tokens in three frames, a token 0 and a token V inside a hypothesis (ldv > V: an unguarded index would stay
    inside the buffer and show as a wrong number), a length above Lmax, utterances of one and of no frame."""
    V, Lmax = 7, 6
    hyps = _pad_fill(12, 7, V)                                     # hyp_ld = 7: row 10 really holds seven tokens
    rows = {0: [1, 2, 3, 4], 1: [1, 2, 3, 5], 2: [2, 2, 3], 3: None,
            4: [], 5: [4, 4, 4], 6: [1, 0, 2], 7: [1, V, 2],
            8: [3], 9: [3, 4], 10: [1, 2, 3, 4, 5, 6, 1], 11: [6, 5, 6]}
    lens = []
    for r in range(12):
        if rows[r] is None:
            lens.append(-1)
            continue
        hyps[r, : len(rows[r])] = torch.tensor(rows[r], dtype=torch.long)
        lens.append(len(rows[r]))
    c = Case(3, 4, 12, V, 8, Lmax, list(hlens), hyps, lens, 21)
    want_bad = {(12, 3, 1): [0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1], (9, 0, 3): [0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0]}[hlens]
    assert c.bad.tolist() == [bool(x) for x in want_bad]           # the yardstick's rule, spelled out
    _check(c)


@pytest.mark.parametrize("hlens", [(1, 2), (32, 33), (34, 64), (65, 70)])
def test_lengths_at_the_recursion_chunk_edges(hlens):
    """(2, 16, 70, 37, 39, 9): the recursion fetches 32 frames at a time; ldv = 39 puts the rows off every alignment."""
    _check(_random_case(2, 16, 70, 37, 39, 9, list(hlens), 31, 0, 9))


@pytest.mark.parametrize("shape,lo,hi", [
    ((2, 10, 120, 3246, 3248, 40), 15, 35),                        # the bench vocabulary
    ((1, 3, 40, 9000, 9000, 5), 3, 5),                             # the row passes through LDS in three pieces
    ((1, 3, 300, 100, 100, 140), 120, 140),                        # 281 states: several per lane
    ((1, 2, 520, 50, 52, 255), 250, 255),                          # the state limit
    ((2, 64, 20, 11, 12, 4), 0, 4),                                # the group limit; every hypothesis shares labels
])
def test_shapes_where_a_mechanism_changes(shape, lo, hi):
    B, group, T, V, ldv, Lmax = shape
    hlens = [T, max(T // 3, 8)][:B]                                # (8 frames hold 4 tokens and their repeats)
    fixed = None
    if V == 9000:
        fixed = [5, 4, 5]
    if Lmax == 255:
        fixed = [255, 250]
    c = _random_case(B, group, T, V, ldv, Lmax, hlens, 41 + Lmax, lo, hi, missing=group > 3, fixed_lens=fixed)
    if V == 9000:                                                  # labels in every piece of the row, one of them in two slots
        c.hyps[0, :5] = torch.tensor([5, 4097, 8500, 4095, 8999], dtype=torch.int32)
        c.hyps[1, :4] = torch.tensor([8999, 4096, 8191, 8192], dtype=torch.int32)
        c = Case(B, group, T, V, ldv, Lmax, hlens, c.hyps, c.lens, 77)
    assert (~c.bad).sum() >= c.R - B * 2
    _check(c)


def test_group_of_one_is_the_fused_ctc_loss():
    """group = 1: logp = -nll of oe_ctc_loss_fused within 1e-3, and with g = -1 dlogits is the loss's gradient."""
    _group_of_one((3, 50, 29, 32, 12), [50, 31, 17], 3, 12)


def test_group_of_one_is_the_fused_ctc_loss_at_a_long_utterance():
    """(B, T, V, ldv, Lmax) = (2, 1500, 64, 64, 200): |nll| in the thousands, the same bounds."""
    _group_of_one((2, 1500, 64, 64, 200), [1500, 700], 150, 200)


def _group_of_one(shape, hlens, lo, hi):
    B, T, V, ldv, Lmax = shape
    c = _random_case(B, 1, T, V, ldv, Lmax, hlens, 51, lo, hi, missing=False)
    g = torch.full((B,), -1.0)
    logp, dl = _device_run(c, g=g)
    buf = torch.full((B, T, ldv), 0.25, device=DEV)
    buf[..., :V] = c.logits.to(DEV)
    nll = torch.empty(B, device=DEV)
    tot = torch.empty(1, device=DEV)
    dref = torch.full((B, T, ldv), SENT, device=DEV)
    ws = torch.empty(hip.lib().oe_ctc_workspace_floats(B, T, Lmax), device=DEV)
    hip.call("oe_ctc_loss_fused", buf, ldv, B, T, V, c.hlens.to(DEV), c.hyps[:, :Lmax].contiguous().to(DEV), Lmax, c.lens.to(DEV), 1.0, None,
             nll, tot, dref, ws)
    torch.cuda.synchronize()
    assert not c.bad.any()
    assert (logp + nll.cpu()).abs().max() < 1e-3
    dref = dref.cpu()[..., :V]
    assert ((dl[..., :V] - dref).abs() <= 2e-5 + 2e-3 * dref.abs()).all()


def test_score_and_grad_replay_from_a_graph_with_the_eager_bits():
    c = _random_case(2, 4, 40, 23, 24, 8, [40, 22], 61, 2, 8)
    logp_e, dl_e = _device_run(c)
    buf = torch.full((c.B, c.T, c.ldv), 0.25, device=DEV)
    buf[..., : c.V] = c.logits.to(DEV)
    dl = torch.full((c.B, c.T, c.ldv), SENT, device=DEV)
    logp = torch.full((c.R,), SENT, device=DEV)
    lib = hip.lib()
    ws = torch.empty(lib.oe_ctc_nbest_workspace_bytes(c.B, c.T, c.group, c.Lmax), dtype=torch.uint8, device=DEV)
    saved = torch.empty(lib.oe_ctc_nbest_saved_bytes(c.B, c.T, c.group, c.Lmax), dtype=torch.uint8, device=DEV)
    hyps, g = c.hyps.to(DEV), c.g.to(DEV)
    args = (buf, c.ldv, c.B, c.T, c.V, c.hlens.to(DEV), hyps, hyps.shape[1], c.lens.to(DEV), c.group, c.Lmax)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.call("oe_ctc_nbest_score", *args, logp, saved, ws)
        hip.call("oe_ctc_nbest_grad", *args, logp, g, saved, dl, None)
    dl.fill_(SENT)
    logp.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(logp.cpu().view(torch.int32), logp_e.view(torch.int32))
    assert torch.equal(dl.cpu().view(torch.int32), dl_e.view(torch.int32))


def test_invalid_arguments_are_reported_not_launched():
    lib = hip.lib()
    B, T, V, group, Lmax = 1, 4, 5, 2, 3
    x = torch.zeros(B, T, 8, device=DEV)
    dx = torch.zeros(B, T, 8, device=DEV)
    hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    hy = torch.ones(B * group, Lmax, dtype=torch.int32, device=DEV)
    ln = torch.ones(B * group, dtype=torch.int32, device=DEV)
    lp = torch.zeros(B * group, device=DEV)
    big = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    keep = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p = hip.ptr

    def score(logits=x, ldv=8, group=group, Lmax=Lmax, hyp_ld=Lmax, logp=lp, ws=big, hlens=hl):
        return lib.oe_ctc_nbest_score(p(logits), ldv, B, T, V, p(hlens), p(hy), hyp_ld, p(ln), group, Lmax, p(logp), p(keep), p(ws), None)

    def grad(dlogits=dx, saved=keep, g=lp, group=group, Lmax=Lmax):
        return lib.oe_ctc_nbest_grad(p(x), 8, B, T, V, p(hl), p(hy), Lmax, p(ln), group, Lmax, p(lp), p(g), p(saved), p(dlogits), None, None)

    for call, word in ((functools.partial(score, logits=None), b"null"), (functools.partial(score, logp=None), b"null"),
                       (functools.partial(score, ws=None), b"null"), (functools.partial(score, hlens=None), b"null"),
                       (functools.partial(score, group=0), b"group"), (functools.partial(score, group=65), b"group"),
                       (functools.partial(score, Lmax=256, hyp_ld=256), b"Lmax"), (functools.partial(score, Lmax=-1), b"Lmax"),
                       (functools.partial(score, ldv=4), b"ldv"), (functools.partial(score, hyp_ld=2), b"hyp_ld"),
                       (functools.partial(grad, dlogits=x), b"alias"), (functools.partial(grad, dlogits=None), b"null"),
                       (functools.partial(grad, saved=None), b"null"), (functools.partial(grad, g=None), b"null"),
                       (functools.partial(grad, group=65), b"group")):
        rc = call()
        assert rc != 0 and word in lib.oe_last_error(), (call, rc, lib.oe_last_error())
    assert score() == 0 and grad() == 0
    torch.cuda.synchronize()


def test_ops_gradient_of_the_mwer_loss_matches_the_yardstick():
    from openeat_amd.utils.mwer import mwer_loss
    c = _random_case(2, 4, 20, 11, 11, 5, [20, 13], 71, 1, 5)
    gen = torch.Generator().manual_seed(72)
    errors = torch.randint(0, 6, (c.B, c.group), generator=gen).float()
    x = c.logits.to(DEV).requires_grad_(True)
    hyps = c.hyps[:, : c.Lmax].contiguous().to(DEV)
    logp = ops.ctc_nbest_logp(x, c.hlens.to(DEV), hyps, c.lens.to(DEV), c.group)
    assert logp.shape == (c.B, c.group)
    with torch.no_grad():                                          # no gradient asked for: the same bits, nothing saved
        assert torch.equal(ops.ctc_nbest_logp(x.detach(), c.hlens.to(DEV), hyps, c.lens.to(DEV), c.group), logp.detach())
    exists = torch.isfinite(logp.detach())
    assert torch.equal(exists.cpu().view(-1), ~c.bad)
    loss, _ = mwer_loss(logp, errors.to(DEV), exists)
    loss.sum().backward()
    xr = c.logits.double().requires_grad_(True)
    lpr = ref.nbest_logp(xr, c.hlens.tolist(), c.hyps[:, : c.Lmax], c.lens, c.group)
    lr, _ = ref.mwer(lpr, errors.double(), torch.isfinite(lpr.detach()))
    lr.sum().backward()
    assert torch.allclose(loss.detach().cpu().double(), lr.detach(), rtol=1e-4, atol=1e-4)
    lp0 = lpr.detach().clone().requires_grad_(True)
    (w,) = torch.autograd.grad(ref.mwer(lp0, errors.double(), torch.isfinite(lp0.detach()))[0].sum(), lp0)
    tol = 2e-5 * torch.nan_to_num(w).abs().sum(1).clamp(min=1.0).view(c.B, 1, 1) + 2e-3 * xr.grad.abs()
    assert xr.grad.abs().max() > 1e-3
    assert ((x.grad.cpu().double() - xr.grad).abs() <= tol).all()
