"""CPU: the yardstick of the n-best CTC scorer (tests/ctc_nbest_ref.py) against brute-force enumeration, and
openeat_amd.utils.mwer.mwer_loss against the restated formula."""
import itertools
import math

import torch

import ctc_nbest_ref as ref


def _collapse(path):
    out, prev = [], -1
    for c in path:
        if c != prev and c != 0:
            out.append(c)
        prev = c
    return tuple(out)


def test_yardstick_logp_is_the_sum_over_all_alignments():
    """T <= 5, V = 3: every one of the V^T alignments is enumerated.  Hypotheses: plain, a repeat, the empty one, one that
    does not fit its frames (a repeat needs a blank between), a missing slot; an utterance shorter than the tensor."""
    V, T, group = 3, 5, 5
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(2, T, V, generator=g, dtype=torch.float64) * 2
    hlens = [5, 3]
    hyps = torch.tensor([[1, 2, 1], [1, 1, 2], [2, 2, 2], [2, 1, 1], [1, 2, 2],
                         [2, 1, 2], [1, 1, 2], [1, 2, 1], [2, 2, 1], [1, 1, 1]])
    lens = torch.tensor([3, 3, 0, 1, -1, 2, 2, 0, 3, 2])      # padding behind a length: valid ids that would change the answer
    got = ref.nbest_logp(logits, hlens, hyps, lens, group)
    p = torch.softmax(logits, -1)
    for r in range(10):
        b, L = r // group, int(lens[r])
        Tb = hlens[b]
        tot = 0.0
        if L >= 0:
            want = tuple(int(x) for x in hyps[r, :L])
            for path in itertools.product(range(V), repeat=Tb):
                if _collapse(path) == want:
                    tot += math.prod(float(p[b, t, c]) for t, c in enumerate(path))
        if tot == 0.0:
            assert got[b, r % group] == -float("inf"), (r, got[b, r % group])
        else:
            assert abs(float(got[b, r % group]) - math.log(tot)) < 1e-10, (r, float(got[b, r % group]), math.log(tot))
    # rows 8 (2,2,1 in 3 frames: needs 4) and 9 (1,1 in 3 frames: fits exactly) bracket the repeat rule; row 4 is missing
    assert got[1, 3] == -float("inf") and torch.isfinite(got[1, 4]) and got[0, 4] == -float("inf")


def test_mwer_loss_is_the_restated_formula_and_differentiable():
    from openeat_amd.utils.mwer import mwer_loss
    g = torch.Generator().manual_seed(12)
    B, N = 4, 5
    logp = (torch.randn(B, N, generator=g, dtype=torch.float64) * 3 - 20).requires_grad_(True)
    errors = torch.randint(0, 9, (B, N), generator=g).double()
    exists = torch.ones(B, N, dtype=torch.bool)
    exists[1, 2] = False
    exists[2, :] = False                                      # an utterance without any entry
    exists[3, 1:] = False                                     # a single entry: loss 0, expected errors = its own
    loss, exp = mwer_loss(logp, errors, exists)
    want_loss, want_exp = ref.mwer(logp.detach(), errors, exists)
    assert torch.allclose(loss, want_loss, rtol=0, atol=1e-12) and torch.allclose(exp, want_exp, rtol=0, atol=1e-12)
    ld, ed = loss.detach(), exp.detach()
    assert ld[2] == 0 and ed[2] == 0 and abs(float(ld[3])) < 1e-15 and abs(float(ed[3]) - float(errors[3, 0])) < 1e-12
    assert torch.autograd.gradcheck(lambda x: mwer_loss(x, errors, exists)[0], (logp,), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda x: mwer_loss(x, errors, exists)[1], (logp,), eps=1e-6, atol=1e-6)
    # what a missing slot holds never matters: -inf likelihood, NaN errors
    lp2 = logp.detach().clone()
    lp2[~exists] = -float("inf")
    lp2.requires_grad_(True)
    er2 = errors.clone()
    er2[~exists] = float("nan")
    loss2, exp2 = mwer_loss(lp2, er2, exists)
    (g2,) = torch.autograd.grad(loss2.sum() + exp2.sum(), lp2)
    assert torch.isfinite(loss2).all() and torch.isfinite(exp2).all() and torch.isfinite(g2).all()
    assert torch.equal(loss2, loss.detach()) and (g2[~exists] == 0).all()


def test_mwer_gradient_rows_of_the_yardstick_sum_to_zero():
    """The MWER weights d loss / d logp sum to zero per utterance, so the dense softmax term of the gradient cancels and
    every row of d loss / d logits sums to 0 (the occupancies of a frame sum to 1)."""
    from openeat_amd.utils.mwer import mwer_loss
    g = torch.Generator().manual_seed(13)
    B, T, V, group = 2, 9, 6, 4
    logits = torch.randn(B, T, V, generator=g, dtype=torch.float64)
    hlens = [9, 6]
    hyps = torch.randint(1, V, (B * group, 4), generator=g)
    lens = torch.tensor([3, 2, 4, -1, 0, 1, 4, 2])
    errors = torch.randint(0, 5, (B, group), generator=g).double()
    x = logits.clone().requires_grad_(True)
    logp = ref.nbest_logp(x, hlens, hyps, lens, group)
    exists = torch.isfinite(logp.detach())
    assert exists.sum() == 7
    lp = logp.detach().clone().requires_grad_(True)
    (w,) = torch.autograd.grad(mwer_loss(lp, errors, exists)[0].sum(), lp)
    assert w[exists].abs().max() > 1e-3 and (w.sum(1).abs() < 1e-12).all()
    _, dx = ref.nbest_grad(logits, hlens, hyps, lens, group, w)
    assert dx.abs().max() > 1e-4 and dx.sum(-1).abs().max() < 1e-12
    assert (dx[1, 6:] == 0).all()
