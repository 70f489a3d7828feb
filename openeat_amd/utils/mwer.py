"""Minimum word error rate (MWER) loss over n-best lists (Prabhavalkar et al. 2018): the expected number of errors under the
hypotheses' likelihoods renormalised over the list.  Plain torch on whatever device the inputs live on; the likelihoods come
from ops.ctc_nbest_logp, the error counts from ops.edit_distance (ASRModel.forward_mwer)."""
import torch


def mwer_loss(logp: torch.Tensor, errors: torch.Tensor, exists: torch.Tensor):
    """logp (B, N) the hypotheses' log-likelihoods, errors (B, N) their error counts, exists (B, N) bool.
    P = softmax of logp over the existing entries (a missing entry has probability 0, whatever its logp and errors hold:
    -inf and NaN included, in forward and in backward); Wbar = the mean of errors over the existing entries.
    -> loss (B) = sum_n P_n (W_n - Wbar) and expected_errors (B) = sum_n P_n W_n; an utterance without entries gives 0."""
    exists = exists.bool()
    zero = torch.zeros((), dtype=logp.dtype, device=logp.device)
    # missing entries are replaced before any arithmetic, so neither their values nor their gradients can be inf or NaN
    lp = torch.where(exists, logp, zero)
    w = torch.where(exists, errors.to(logp.dtype), zero)
    top = torch.where(exists, lp, torch.full_like(lp, -float("inf"))).amax(dim=1, keepdim=True)
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top)).detach()
    e = torch.where(exists, torch.exp(lp - top), zero)
    denom = e.sum(dim=1, keepdim=True)
    p = e / torch.where(denom > 0, denom, torch.ones_like(denom))
    n = exists.sum(dim=1, keepdim=True).to(logp.dtype)
    wbar = w.sum(dim=1, keepdim=True) / n.clamp(min=1)
    loss = (p * torch.where(exists, w - wbar, zero)).sum(dim=1)
    return loss, (p * w).sum(dim=1)
