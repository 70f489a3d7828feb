"""The yardstick of oe_ctc_nbest_score / oe_ctc_nbest_grad and of the MWER loss on top of them: torch's own CTC loss in
float64 on the CPU, over the log-softmax of the logits repeated `group` times - the expanded form the grouped kernels
replace.  The infeasibility rule of include/openeat_hip.h is restated in plain Python and applied with masked_fill (with
zero_infinity=False torch's gradient of an infeasible row is NaN; with the mask it is exactly 0).  Independent of the code under
test."""
import torch
import torch.nn.functional as F


def infeasible_rows(hlens, hyps, hyp_lens, group, V, Lmax, T):
    """-> (R) bool by the rule: missing slot, length > Lmax, no frames, fewer frames than length + adjacent repeats, a token
    within the length outside 1..V-1."""
    out = []
    for r, L in enumerate(int(x) for x in hyp_lens):
        Tb = min(max(int(hlens[r // group]), 0), T)
        bad = L < 0 or L > Lmax or Tb == 0
        if not bad:
            toks = [int(x) for x in hyps[r, :L]]
            bad = any(c < 1 or c > V - 1 for c in toks) or Tb < L + sum(1 for i in range(1, L) if toks[i] == toks[i - 1])
        out.append(bad)
    return torch.tensor(out, dtype=torch.bool)


def nbest_logp(logits, hlens, hyps, hyp_lens, group):
    """logits (B, T, V) float64 (may require grad), hlens (B), hyps (R, Lmax), hyp_lens (R) -> logp (B, group) float64, -inf at
    the infeasible rows; differentiable with respect to logits."""
    B, T, V = logits.shape
    R, Lmax = hyps.shape
    assert R == B * group and logits.dtype == torch.float64
    bad = infeasible_rows(hlens, hyps, hyp_lens, group, V, Lmax, T)
    lens = torch.as_tensor(hyp_lens, dtype=torch.long).clone()
    lens[bad] = 0                                        # their result is masked; nothing of them may reach torch's index checks
    tg = torch.as_tensor(hyps, dtype=torch.long).clamp(1, V - 1)
    if Lmax == 0:
        tg = torch.ones(R, 1, dtype=torch.long)
    hl = torch.as_tensor(hlens, dtype=torch.long).clamp(0, T).repeat_interleave(group)
    hl = torch.where(bad, torch.ones_like(hl).clamp(max=T), hl)
    lp = F.log_softmax(logits, dim=-1).repeat_interleave(group, 0).transpose(0, 1)      # (T, R, V)
    nll = F.ctc_loss(lp, tg, hl, lens, blank=0, reduction="none", zero_infinity=True)
    return (-nll).masked_fill(bad, -float("inf")).view(B, group)


def mwer(logp, errors, exists):
    """The MWER formula restated, one utterance at a time: P = softmax of logp over the existing entries, Wbar = the mean of
    errors over them -> (loss (B), expected_errors (B)); an utterance without entries gives 0."""
    loss, exp = [], []
    for b in range(logp.shape[0]):
        idx = [n for n in range(logp.shape[1]) if bool(exists[b, n])]
        if not idx:
            loss.append(logp.new_zeros(()))
            exp.append(logp.new_zeros(()))
            continue
        p = torch.softmax(torch.stack([logp[b, n] for n in idx]), 0)
        w = torch.stack([errors[b, n].to(logp.dtype) for n in idx])
        loss.append((p * (w - w.mean())).sum())
        exp.append((p * w).sum())
    return torch.stack(loss), torch.stack(exp)


def nbest_grad(logits, hlens, hyps, hyp_lens, group, g):
    """-> (logp (B, group), d sum(g * logp) / d logits) in float64; g (B, group), entries at infeasible rows are ignored."""
    x = logits.detach().double().requires_grad_(True)
    logp = nbest_logp(x, hlens, hyps, hyp_lens, group)
    fin = torch.isfinite(logp)
    tot = (torch.where(fin, logp, torch.zeros_like(logp)) * torch.where(fin, g.double(), torch.zeros_like(logp))).sum()
    (dx,) = torch.autograd.grad(tot, x, allow_unused=True)
    return logp.detach(), (torch.zeros_like(x) if dx is None else dx)
