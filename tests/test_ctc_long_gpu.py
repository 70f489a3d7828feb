"""GPU: oe_ctc_loss_fused (raw C ABI) at long, high-loss utterances against torch's CTC loss in FLOAT64 (ctc_long_cases.py).
torch's float32 loss - the yardstick of test_ctc_vs_oracle - drifts with the utterance's negative log-likelihood just as a float32
kernel does, so it cannot judge these shapes.  Tolerances are those of test_ctc_vs_oracle: nll rtol 1e-4 / atol 1e-3; dlogits
rtol 2e-3 / atol 2e-5 * grad_scale * utt_weight.  The padding columns of the logits hold an ordinary number, dlogits is prefilled
with a sentinel, the targets hold valid token ids behind every length."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_long_cases as cases  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from test_gpu_kernels import ctc_form  # noqa: E402,F401  (fixture: the four launch forms)

DEV = "cuda"
SENT = -777.0
FORMS = ((0, 4), (2, 4), (2, 3), (2, 8))        # the settings of ctc_form, for the test that walks them itself


@functools.lru_cache(maxsize=None)
def _case(name):
    """A case and its yardstick, made once for all launch forms (nothing writes to a case)."""
    return {"flat": cases.flat, "peaked": cases.peaked, "row shift": cases.row_shift,
            "one alignment": lambda: cases.single_alignment()[0],
            "bench vocabulary": lambda: cases.random_case(1, 1500, 3246, 200, [1500], [200], 2.0, 1, repeat_at=(11,)),
            "state limit": lambda: cases.random_case(1, 2000, 32, 255, [2000], [255], 8.0, 2, repeat_at=(100,))}[name]()


def _launch(c, ldv, scale=1.0, inplace=False, utt_weight=None, want_grad=True):
    """-> nll (B), loss_sum (1), dlogits (B, T, ldv) or None - on the device."""
    buf = torch.full((c.B, c.T, ldv), 0.25, device=DEV)
    buf[..., : c.V] = c.logits.to(DEV)
    dl = None
    if want_grad:
        dl = buf if inplace else torch.full((c.B, c.T, ldv), SENT, device=DEV)
    nll = torch.full((c.B,), SENT, device=DEV)
    tot = torch.full((1,), SENT, device=DEV)
    ws = torch.empty(hip.lib().oe_ctc_workspace_floats(c.B, c.T, c.Lmax), device=DEV)
    uw = None if utt_weight is None else utt_weight.float().to(DEV)
    hip.call("oe_ctc_loss_fused", buf, ldv, c.B, c.T, c.V, c.hlens.to(DEV), c.ys.to(DEV), c.Lmax, c.ylens.to(DEV), float(scale), uw,
             nll, tot, dl, ws)
    torch.cuda.synchronize()
    return nll, tot, dl


def _errors(c, nll, tot, dl, scale=1.0, utt_weight=None):
    """-> (worst nll err / tol, worst dlogits err / tol) against the float64 yardstick; the comparison runs on the device."""
    want_nll, want_grad = c.yardstick()
    w = torch.ones(c.B, dtype=torch.float64) if utt_weight is None else utt_weight.double()
    nerr = (nll.cpu().double() - want_nll).abs() / (1e-3 + 1e-4 * want_nll.abs())
    want_tot = (w * want_nll).sum()
    terr = (tot.cpu().double()[0] - want_tot).abs() / (1e-3 + 1e-4 * want_tot.abs())
    f = (scale * w).view(c.B, 1, 1).to(DEV)
    if getattr(c, "ref_dev", None) is None:
        c.ref_dev = want_grad.to(DEV)
    want = c.ref_dev * f
    got = dl[..., : c.V].double()
    assert bool(torch.isfinite(got).all())
    gerr = (got - want).abs() / (2e-5 * f + 2e-3 * want.abs())
    return float(torch.maximum(nerr.max(), terr)), float(gerr.max())


def _check(name, ldv, scale=1.0, inplace=False, utt_weight=None):
    c = _case(name)
    nll, tot, dl = _launch(c, ldv, scale, inplace, utt_weight)
    nratio, gratio = _errors(c, nll, tot, dl, scale, utt_weight)
    print(f"{name}: nll {[round(float(x), 1) for x in c.yardstick()[0]]} worst err / tol: nll {nratio:.3g}, dlogits {gratio:.3g}")
    bad = c.infeasible()
    for b in range(c.B):
        Tb = int(c.hlens[b])
        assert bool((dl[b, Tb:, : c.V] == 0).all())                              # padded frames: exact zeros
        if bad[b]:
            assert float(nll[b]) == 0.0 and bool((dl[b, :, : c.V] == 0).all())   # zero_infinity
    if not inplace:
        assert bool((dl[..., c.V:] == SENT).all())                               # columns >= V are not written
    assert nratio <= 1.0 and gratio <= 1.0, (name, nratio, gratio)
    return nll, tot, dl


def test_flat_and_long(ctc_form):
    """(B, T, V, ldv, Lmax) = (2, 1500, 64, 66, 200), randn * 6, hlens (1500, 40): |nll| ~ 15000 nats beside a short utterance in
    the same launch; grad_scale and utterance weights other than 1."""
    _check("flat", 66, scale=0.5, utt_weight=torch.tensor([0.7, 1.3]))


def test_bench_vocabulary_long(ctc_form):
    """(1, 1500, 3246, 3248, 200), randn * 2."""
    _check("bench vocabulary", 3248)


def test_state_limit_long_in_place(ctc_form):
    """(1, 2000, 32, 32, 255), randn * 8, dlogits == logits."""
    _check("state limit", 32, inplace=True)


def test_one_admissible_alignment(ctc_form):
    """261 frames for 255 labels with six adjacent repeats: gradient = softmax - onehot(path) (test_ctc_long_ref.py pins the
    yardstick to that); beside it 262 frames (many alignments) and 260 (infeasible: loss 0, gradient exactly 0)."""
    c, path = _case("one alignment"), cases.single_alignment()[1]
    nll, tot, dl = _check("one alignment", 68)
    occ = torch.softmax(c.logits[0, :261].double(), -1) - dl[0, :261, : c.V].cpu().double()
    onehot = torch.zeros(261, c.V, dtype=torch.float64)
    onehot[torch.arange(261), path] = 1.0
    assert float((occ - onehot).abs().max()) <= 2e-5 + 2e-3                      # the tolerance at an occupancy of 1


def test_peaked_control(ctc_form):
    """The flat shape with a +14 peak along a valid alignment: nll ~ 4 nats.  No drift to speak of: float32 state passes this."""
    assert float(_case("peaked").yardstick()[0][0]) < 20.0
    _check("peaked", 66)


def test_row_shift(ctc_form):
    """(3, 70, 37, 40, 5): +3e4 on every logit of one utterance, -3e4 on another's."""
    _check("row shift", 40)


def test_ladder():
    """T in 248 .. 2000 at the bench vocabulary (B = 1, V = 3246, ldv 3248, randn * 2, L = min(255, T // 6)), seeds 0 - 2, every
    launch form: loss and gradient of every point at the tolerances above.  The table it prints is the one beside
    CTC_F32_MAX_T in csrc/ctc.hip."""
    rows, failed = [], []
    try:
        for T in cases.LADDER_T:
            worst_n = worst_g = 0.0
            for seed in range(3):
                c = cases.ladder_point(T, seed)
                for mode, chunks in FORMS:
                    hip.lib().oe_ctc_config(mode, chunks)
                    nll, tot, dl = _launch(c, 3248)
                    nratio, gratio = _errors(c, nll, tot, dl)
                    worst_n, worst_g = max(worst_n, nratio), max(worst_g, gratio)
                    if nratio > 1.0 or gratio > 1.0 or not bool((dl[..., c.V:] == SENT).all()):
                        failed.append((T, seed, mode, chunks, round(nratio, 3), round(gratio, 3)))
            rows.append((T, float(c.yardstick()[0][0]), worst_n, worst_g))
    finally:
        hip.lib().oe_ctc_config(0, 4)
    print("ladder:  T   nll(seed 2)   worst nll err/tol   worst dlogits err/tol")
    for T, n, a, g in rows:
        print(f"ladder: {T:5d} {n:10.1f} {a:10.3g} {g:10.3g}")
    assert not failed, failed


def test_through_autograd():
    """The flat shape through ops.ctc_head (in place on its own logits buffer, 1 / B folded into grad_scale): the projection is
    the identity, the yardstick reads the logits the op's own GEMM call produces."""
    c0 = _case("flat")
    B, T, V = c0.B, c0.T, c0.V
    x = c0.logits.to(DEV).requires_grad_(True)
    w = torch.eye(V, device=DEV).requires_grad_(True)
    b = torch.zeros(V, device=DEV).requires_grad_(True)
    seen = torch.empty(B * T, V, device=DEV)
    hip.gemm(x.detach().view(-1, V), w.detach(), seen, B * T, V, V, lda=V, ldb=V, ldc=V, bias=b.detach())
    torch.cuda.synchronize()
    c = cases.Case(seen.cpu().view(B, T, V), c0.hlens, c0.ys, c0.ylens)
    loss = ops.ctc_head(x, w, b, c.hlens.to(DEV), c.ys.to(DEV), c.ylens.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    want_nll, want_grad = c.yardstick()
    want_loss = float(want_nll.sum()) / B
    assert abs(float(loss) - want_loss) <= 1e-3 + 1e-4 * abs(want_loss)
    want = want_grad / B                                                          # d loss / d x = d loss / d logits: w is the identity
    ratio = ((x.grad.cpu().double() - want).abs() / (2e-5 / B + 2e-3 * want.abs())).max()
    print(f"through autograd: loss {float(loss):.6g} (yardstick {want_loss:.6g}), worst x.grad err / tol {float(ratio):.3g}")
    assert float(ratio) <= 1.0


def test_bits_are_equal_with_and_without_the_gradient_and_from_run_to_run():
    c = _case("flat")
    w = torch.tensor([0.7, 1.3])
    nll0, tot0, none = _launch(c, 66, 0.5, utt_weight=w, want_grad=False)
    assert none is None
    nll1, tot1, dl1 = _launch(c, 66, 0.5, utt_weight=w)
    nll2, tot2, dl2 = _launch(c, 66, 0.5, utt_weight=w)
    for n, t in ((nll0, tot0), (nll2, tot2)):
        assert torch.equal(n.view(torch.int32), nll1.view(torch.int32)) and torch.equal(t.view(torch.int32), tot1.view(torch.int32))
    assert torch.equal(dl2.view(torch.int32), dl1.view(torch.int32))


def test_replay_from_a_graph_with_the_eager_bits():
    c = _case("flat")
    ldv = 66
    nll_e, tot_e, dl_e = _launch(c, ldv, 0.5)
    buf = torch.full((c.B, c.T, ldv), 0.25, device=DEV)
    buf[..., : c.V] = c.logits.to(DEV)
    dl = torch.full((c.B, c.T, ldv), SENT, device=DEV)
    nll = torch.full((c.B,), SENT, device=DEV)
    tot = torch.full((1,), SENT, device=DEV)
    ws = torch.empty(hip.lib().oe_ctc_workspace_floats(c.B, c.T, c.Lmax), device=DEV)
    hl, ys, yl = c.hlens.to(DEV), c.ys.to(DEV), c.ylens.to(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.call("oe_ctc_loss_fused", buf, ldv, c.B, c.T, c.V, hl, ys, c.Lmax, yl, 0.5, None, nll, tot, dl, ws)
    dl.fill_(SENT)
    nll.fill_(SENT)
    tot.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(nll.view(torch.int32), nll_e.view(torch.int32)) and torch.equal(tot.view(torch.int32), tot_e.view(torch.int32))
    assert torch.equal(dl.view(torch.int32), dl_e.view(torch.int32))
