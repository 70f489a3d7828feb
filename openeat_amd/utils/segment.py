"""Host side of long-form CTC segmentation (ASRModel.ctc_segment; CTC segmentation, Kuerzinger et al. 2020): the plan that
cuts a recording into overlapping encoder windows, and the per-utterance statistics of a segmented path.  No kernel here: the
plan is pure Python, the statistics are tensor operations on whichever device holds the path."""
from typing import List, Sequence, Tuple

import torch


def encoder_frames(n_feat: int, rate: int, right_context: int) -> int:
    """Encoder frames whose receptive field [rate * i, rate * i + right_context] lies inside n_feat feature frames."""
    return 0 if n_feat < right_context + 1 else (n_feat - right_context - 1) // rate + 1


def window_plan(n_feat: int, window: int, margin: int, rate: int, right_context: int) -> List[Tuple[int, int, int, int, int]]:
    """Windows for encoding a recording of n_feat feature frames piecewise -> [(feat_from, feat_to, keep_from, keep_to, out_from)].

    T' = encoder_frames(n_feat, rate, right_context).  The kept spans [k0, k1) of `window` encoder frames tile [0, T')
    exactly; each is computed on [c0, c1) = [max(0, k0 - margin), min(T', k1 + margin)), i.e. from the features
    [rate * c0, rate * (c1 - 1) + right_context + 1) = [feat_from, feat_to), which yield exactly c1 - c0 encoder frames under the
    Conv2d subsamplings (4: 3/2 3/2, 6: 3/2 5/3, 8: 3/2 3/2 3/2) and the linear one (rate 1, right_context 0).  Of those frames
    [keep_from, keep_to) = [k0 - c0, k1 - c0) go to the output rows [out_from, out_from + keep_to - keep_from), out_from = k0.
    `rate` and `right_context` are the attributes the subsampling modules carry.  (Conv2dSubsampling6 carries right_context
    14 where its receptive field needs 10: for some lengths a plain pass yields one frame more than T'; the plan never asks
    for features that do not exist.)"""
    if window < 1:
        raise ValueError(f"window_plan: window {window} < 1")
    if margin < 0:
        raise ValueError(f"window_plan: margin {margin} < 0")
    n_enc = encoder_frames(n_feat, rate, right_context)
    if n_enc < 1:
        raise ValueError(f"window_plan: {n_feat} feature frames are fewer than the {right_context + 1} one encoder frame needs")
    plan = []
    for k0 in range(0, n_enc, window):
        k1 = min(n_enc, k0 + window)
        c0, c1 = max(0, k0 - margin), min(n_enc, k1 + margin)
        plan.append((rate * c0, rate * (c1 - 1) + right_context + 1, k0 - c0, k1 - c0, k0))
    return plan


def segment_stats(path_logp: torch.Tensor, tok_start: torch.Tensor, tok_end: torch.Tensor, offsets: Sequence[int], win: int = 30):
    """Per utterance of one segmented recording -> tensors (start_frame (U) int64, end_frame (U) int64, mean_logp (U) float64,
    min_logp (U) float64) on the inputs' device.

    path_logp (T), tok_start / tok_end (L) as ops.ctc_segment returns them for the recording; offsets: the utterances' label
    offsets, strictly ascending from 0 to L (utterance u owns the labels [offsets[u], offsets[u+1])).  start = tok_start of the
    utterance's first label, end = tok_end of its last; mean_logp = the float64 mean of path_logp[start .. end]; min_logp = the
    minimum over consecutive blocks of `win` frames from `start` (the last one may be partial) of the block's mean - the
    confidence of CTC segmentation is exp(min_logp).  Tensor operations only (one float64 cumsum): no loop over frames."""
    offsets = [int(o) for o in offsets]
    L = int(tok_start.shape[0])
    if win < 1:
        raise ValueError(f"segment_stats: win {win} < 1")
    if len(offsets) < 2 or offsets[0] != 0 or offsets[-1] != L or any(b <= a for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"segment_stats: offsets must ascend strictly from 0 to {L} (an utterance without labels has no segment): {offsets}")
    dev = path_logp.device
    T = int(path_logp.shape[0])
    off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    start = tok_start.to(torch.int64)[off[:-1]]
    end = tok_end.to(torch.int64)[off[1:] - 1]
    cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), path_logp.to(torch.float64).cumsum(0)])
    mean = (cs[end + 1] - cs[start]) / (end - start + 1).to(torch.float64)
    k = torch.arange((T + win - 1) // win, dtype=torch.int64, device=dev)
    lo = start[:, None] + k[None, :] * win                                   # (U, blocks): a block's first frame
    live = lo <= end[:, None]
    lo = torch.where(live, lo, start[:, None])
    hi = torch.minimum(lo + win, end[:, None] + 1)
    blk = (cs[hi] - cs[lo]) / (hi - lo).to(torch.float64)
    blk = torch.where(live, blk, torch.full_like(blk, float("inf")))
    return start, end, mean, blk.min(dim=1).values
