"""CPU: the float64 yardstick of the long-utterance CTC tests (ctc_long_cases.Case.yardstick: torch's CTC loss in float64)
pinned where the answer is known without it - a target whose frames admit exactly one alignment - and against the loop-level
float64 restatement oracle/ctc_np.py on a small batch."""
import numpy as np
import torch

import ctc_long_cases as cases
from oracle import ctc_np


def test_one_admissible_alignment_gives_one_hot_occupancies():
    """occupancy = softmax - gradient.  Utterance 0: onehot(path) to 1e-9; every live row of the feasible utterances sums to 1
    to 1e-9; the infeasible utterance: loss 0, gradient exactly 0.  (torch's float32 loss does not meet this: its occupancies
    reach 1.0005 and row maxima fall to 0.9987.)"""
    c, path = cases.single_alignment()
    assert c.infeasible().tolist() == [False, False, True]
    nll, grad = c.yardstick()
    occ = torch.softmax(c.logits.double(), -1) - grad
    T0 = int(c.hlens[0])
    onehot = torch.zeros(T0, c.V, dtype=torch.float64)
    onehot[torch.arange(T0), path] = 1.0
    err = (occ[0, :T0] - onehot).abs().max()
    print(f"one alignment: max |occ - onehot| {float(err):.3g}, occupancy maximum - 1 = {float(occ[0].max() - 1):.3g}")
    assert err <= 1e-9
    lp = torch.log_softmax(c.logits[0, :T0].double(), -1)
    assert abs(float(nll[0]) + float(lp[torch.arange(T0), path].sum())) <= 1e-9 * float(nll[0])     # the loss is the path's
    for b in (0, 1):
        Tb = int(c.hlens[b])
        assert (occ[b, :Tb].sum(-1) - 1.0).abs().max() <= 1e-9
        assert bool((grad[b, Tb:] == 0).all())
    assert float(nll[2]) == 0.0 and bool((grad[2] == 0).all())
    assert float(nll[1]) > 0


def test_yardstick_agrees_with_the_loop_level_oracle():
    """(B, T, V, L) = (2, 40, 11, 6), ragged, a repeat: 1e-10."""
    c = cases.random_case(2, 40, 11, 6, [40, 23], [6, 4], 2.0, 5, repeat_at=(2,))
    nll, grad = c.yardstick()
    n2, g2 = ctc_np.ctc_nll_and_grad(c.logits.numpy(), c.hlens.numpy(), c.ys.numpy(), c.ylens.numpy())
    np.testing.assert_allclose(nll.numpy(), n2, rtol=0, atol=1e-10)
    np.testing.assert_allclose(grad.numpy(), g2, rtol=0, atol=1e-10)
    assert np.abs(g2).max() > 0.1
