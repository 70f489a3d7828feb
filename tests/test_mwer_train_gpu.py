"""GPU: ASRModel.forward_mwer / ASRModel.ctc_nbest / Executor.train(args["mwer"]) on a tiny conformer against the float64
yardstick tests/ctc_nbest_ref.py (run on the model's own logits) and tests/edit_distance_ref.py, and at the row count where the
row-gated fusions of ops.py are on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_nbest_ref as ref  # noqa: E402
import edit_distance_ref  # noqa: E402
from openeat_amd import hip  # noqa: E402
from openeat_amd.models.asr_model import ASRModel  # noqa: E402
from openeat_amd.utils.executor import Executor  # noqa: E402

DEV = "cuda"
V, NBEST = 20, 4
N_FEATS = [400, 250]
TLENS = [12, 7]


def _model(ctc_scale=12.0):
    """2 blocks, d = 32, V = 20, random weights, dropout 0; the CTC projection is scaled up so that the frames have opinions."""
    torch.manual_seed(5)
    model = ASRModel(80, V, encoder_num_blocks=2, decoder_num_blocks=1, r_decoder_num_blocks=1, d_model=32, attention_heads=4,
                     linear_units=64, dropout_rate=0.0, cnn_module_kernel=15, reverse_weight=0.3)
    with torch.no_grad():
        model.ctc.ctc_lo.weight.mul_(ctc_scale)
    return model.to(DEV)


def _batch(seed=6):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(N_FEATS), max(N_FEATS), 80, generator=g)
    for b, n in enumerate(N_FEATS):
        feats[b, n:] = 0.0
    tgt = torch.full((len(TLENS), max(TLENS)), -1, dtype=torch.int32)
    for b, n in enumerate(TLENS):
        tgt[b, :n] = torch.randint(1, V - 1, (n,), generator=g, dtype=torch.int32)
    return dict(features=feats.to(DEV), features_length=torch.tensor(N_FEATS, dtype=torch.int32, device=DEV),
                targets=tgt.to(DEV), targets_length=torch.tensor(TLENS, dtype=torch.int32, device=DEV))


def _ref_errors(batch, info):
    """sub + del + ins of every existing n-best entry by the plain-Python edit distance -> (B, NBEST) float64 (0 where missing)."""
    tgt, tl = batch["targets"].cpu(), batch["targets_length"].cpu()
    pre, plen = info["prefixes"].cpu(), info["plen"].cpu()
    out = torch.zeros(tgt.shape[0], NBEST, dtype=torch.float64)
    for r in range(plen.numel()):
        if plen[r] >= 0:
            (_, s, d, i), _ = edit_distance_ref.edit_distance(tgt[r // NBEST, : tl[r // NBEST]].tolist(), pre[r, : plen[r]].tolist())
            out[r // NBEST, r % NBEST] = s + d + i
    return out


def test_base_loss_and_errors_of_forward_mwer():
    model, batch = _model().eval(), _batch()
    with torch.no_grad():
        loss, info = model.forward_mwer(**batch, nbest=NBEST)
        want, acc = model(**batch)
    torch.cuda.synchronize()
    assert set(info) >= {"loss_mwer", "loss_base", "acc", "expected_errors", "logp", "errors", "prefixes", "plen"}
    assert abs(float(info["loss_base"]) - float(want)) <= 1e-6 * abs(float(want)), (float(info["loss_base"]), float(want))
    assert float(info["acc"]) == float(acc)
    assert abs(float(loss) - (float(info["loss_mwer"]) + 0.01 * float(want))) <= 1e-5 * abs(float(loss))
    # the error counts are exactly the plain-Python ones
    plen = info["plen"].cpu().view(-1, NBEST)
    assert (plen >= 0).sum() >= 4 and info["errors"].shape == (2, NBEST)
    errs = _ref_errors(batch, info)
    assert torch.equal(info["errors"].cpu().double()[plen >= 0], errs[plen >= 0])
    assert errs.max() > 0
    with pytest.raises(ValueError):
        model.forward_mwer(**batch, nbest=17)


def test_mwer_loss_and_projection_gradient_match_the_yardstick():
    model, batch = _model().eval(), _batch()
    loss, info = model.forward_mwer(**batch, nbest=NBEST, ce_weight=0.0)
    loss.backward()
    with torch.no_grad():
        enc, mask, _ = model._encode(batch["features"], batch["features_length"])
        logits = model.ctc.logits(enc)
    torch.cuda.synchronize()
    lens = mask.squeeze(1).sum(1).cpu()
    T = logits.shape[1]
    pre, plen = info["prefixes"].cpu()[:, : min(T, 255)], info["plen"].cpu()
    errors = _ref_errors(batch, info)
    x = logits.cpu().double().requires_grad_(True)
    logp = ref.nbest_logp(x, lens.tolist(), pre, plen, NBEST)
    exists = torch.isfinite(logp.detach())
    assert torch.equal(exists, torch.isfinite(info["logp"].cpu())) and exists.sum() >= 4
    per_utt, exp = ref.mwer(logp, errors, exists)
    per_utt.mean().backward()
    want = per_utt.detach().mean()
    # the weights of the hypotheses, d loss / d logp: what a logp error of (1e-3 + 1e-4 |logp|) can move the loss by
    lp0 = logp.detach().clone().requires_grad_(True)
    (w,) = torch.autograd.grad(ref.mwer(lp0, errors, exists)[0].mean(), lp0)
    w = torch.nan_to_num(w)
    ltol = float((w.abs() * (1e-3 + 1e-4 * torch.nan_to_num(logp.detach(), neginf=0.0).abs())).sum()) + 1e-6
    print(f"loss_mwer {float(info['loss_mwer']):.6g} yardstick {float(want):.6g} tol {ltol:.3g}; expected errors {info['expected_errors'].tolist()} / {exp.tolist()}")
    assert abs(float(info["loss_mwer"]) - float(want)) <= ltol
    assert float(w.abs().max()) > 1e-4                                  # the lists really pull on the logits
    # d loss / d W = dlogits^T h: the dlogits tolerance (rtol 2e-3, atol 2e-5 * max(1, sum |w|)) carried through the projection
    h = enc.cpu().double()
    dl = x.grad
    tol_dl = 2e-5 * w.abs().sum(1).clamp(min=1.0).view(-1, 1, 1) + 2e-3 * dl.abs()
    want_dw = torch.einsum("btv,btk->vk", dl, h)
    tol_dw = torch.einsum("btv,btk->vk", tol_dl, h.abs())
    got = model.ctc.ctc_lo.weight.grad.cpu().double()
    err = (got - want_dw).abs()
    print(f"dW: max err {float(err.max()):.3g}, max |ref| {float(want_dw.abs().max()):.3g}, worst err / tol {float((err / tol_dw).max()):.3g}")
    assert want_dw.abs().max() > 1e-4 and (err <= tol_dw).all()


def test_ctc_nbest_lists_carry_the_exact_likelihood():
    model, batch = _model().eval(), _batch()
    lists = model.ctc_nbest(batch["features"], batch["features_length"], NBEST)
    with torch.no_grad():
        _, _, pre, plen, _, _, _ = model._rescore_stage1(batch["features"], batch["features_length"], hip.PrefixSearch(NBEST))
    pre, plen = pre.cpu(), plen.cpu()
    assert len(lists) == 2
    seen = 0
    for b, nb in enumerate(lists):
        rows = [r for r in range(b * NBEST, (b + 1) * NBEST) if plen[r] >= 0]
        assert [list(e[0]) for e in nb] == [pre[r, : plen[r]].tolist() for r in rows]
        for tokens, beam_score, exact in nb:
            assert exact >= beam_score - 1e-3, (tokens, beam_score, exact)      # the beam sums a subset of the same alignments
            assert exact <= 0.0
            seen += 1
    assert seen >= 4
    with pytest.raises(ValueError):
        model.ctc_nbest(batch["features"], batch["features_length"], 17)


def test_forward_mwer_at_the_row_count_of_the_fused_kernels():
    """One encoder block at d = 256 on 18 x 9.3 s = 4176 encoder rows: the row-gated fusions of ops.py are on while encoder_out
    feeds one consumer more than in forward().  The whole batch against its two halves, averaged (tests/test_gpu_width.py's
    tolerances: loss 2e-4, gradient norms 3e-3); the halves score the whole batch's n-best lists."""
    from openeat_amd import ops
    Vw, B, nb = 200, 18, 4
    torch.manual_seed(31)
    model = ASRModel(80, Vw, encoder_num_blocks=1, decoder_num_blocks=1, r_decoder_num_blocks=1, d_model=256, attention_heads=4,
                     linear_units=1024, dropout_rate=0.0, cnn_module_kernel=15, reverse_weight=0.3).to(DEV).eval()
    with torch.no_grad():
        model.ctc.ctc_lo.weight.mul_(6.0)
    g = torch.Generator().manual_seed(32)
    nfr = [930, 900, 870, 930, 800, 760, 930, 910, 650] * 2
    feats = torch.randn(B, 930, 80, generator=g)
    tl = [20 - (b % 9) for b in range(B)]
    tgt = torch.full((B, 20), -1, dtype=torch.int32)
    for b in range(B):
        feats[b, nfr[b]:] = 0.0
        tgt[b, : tl[b]] = torch.randint(1, Vw - 1, (tl[b],), generator=g, dtype=torch.int32)
    feats, nfr_t, tgt, tl_t = feats.to(DEV), torch.tensor(nfr, dtype=torch.int32, device=DEV), tgt.to(DEV), torch.tensor(tl, dtype=torch.int32, device=DEV)
    loss, info = model.forward_mwer(feats, nfr_t, tgt, tl_t, nbest=nb)
    assert B * info["prefixes"].shape[1] >= max(ops.ROWGEMM_MIN_ROWS, ops.FUSED_FFN_MIN_ROWS) == 4096      # encoder rows
    loss.backward()
    whole = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    losses = []
    for lo in (0, 9):
        sl = slice(lo, lo + 9)
        lists = (info["prefixes"][lo * nb: (lo + 9) * nb], info["plen"][lo * nb: (lo + 9) * nb])
        l, inf2 = model.forward_mwer(feats[sl], nfr_t[sl], tgt[sl], tl_t[sl], nbest=nb, nbest_lists=lists)
        (l / 2).backward()
        losses.append(float(l.detach()))
        assert torch.equal(inf2["errors"], info["errors"][sl])
    torch.cuda.synchronize()
    half = sum(losses) / 2
    loss = loss.detach()
    print(f"loss whole {float(loss):.6f} halves {half:.6f}; loss_mwer {float(info['loss_mwer']):.5f}")
    assert abs(float(loss) - half) <= 2e-4 * abs(half), (float(loss), half)
    assert float(info["loss_mwer"]) != 0.0
    bad = []
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        got, want = float(whole[k].norm()), float(p.grad.norm())
        if abs(got - want) > 3e-3 * abs(want) + 1e-6:
            bad.append((k, got, want))
    assert not bad, bad[:10]


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def test_executor_trains_on_the_mwer_loss_when_asked():
    model, b1, b2 = _model(), _batch(6), _batch(8)
    with torch.no_grad():
        want, _ = model.eval()(**b1)
    want = float(want)
    sched = lambda opt: torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)      # noqa: E731
    # without the key: the loop is the likelihood loop it was
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    log = _Log()
    got, _ = Executor().train(log, model, opt, sched(opt), [(["a", "b"], b1)], DEV, {"log_interval": 1})
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert not any("MWER" in line for line in log.lines)
    # with it: two steps on the MWER loss move the parameters
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    log = _Log()
    ex = Executor()
    got, _ = ex.train(log, model, opt, sched(opt), [(["a", "b"], b1), (["c", "d"], b2)], DEV, {"log_interval": 1, "mwer": {"nbest": NBEST, "ce_weight": 0.01}})
    torch.cuda.synchronize()
    assert ex.step == 2 and got == got and abs(got) < 1e6
    assert sum("MWER:" in line and "ExpErr:" in line for line in log.lines) == 2
    moved = [k for k, v in model.state_dict().items() if v.is_floating_point() and not torch.equal(v, before[k])]
    assert "ctc.ctc_lo.weight" in moved and len(moved) > 10
