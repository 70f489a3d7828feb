#!/usr/bin/env python3
"""The LM-fused CTC prefix beam search (oe_ctc_prefix_beam with an n-gram model) against the plain one on the same top-k:
the two instantiations of beam.hip's kernel (GPU box).

  python tools/lm_beam_bench.py           # 64 utterances x 250 frames, beam 10, synthetic n-gram models of order 3 and 5

The top-k comes from random logits over 3246 tokens (randn * 3, blank + 3: peaky frames with frequent blanks, as a CTC
posterior has them) through ops.topk_rows; the models are built from arrays (~1 M n-grams, a table that fits neither LDS nor
the L2), their n-grams chained so that every order is matched by extensions of listed contexts.  Only the kernels are timed:
outputs and workspace are allocated once.  HIP events, median of 20 calls after 3 warm-up calls, three alternating runs
(the machine is shared); the middle run is reported, as microseconds per call and per frame, and the ratio fused / plain."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402

DEV = "cuda"
V, B, T, BEAM = 3246, 64, 250, 10


def timed(fn, n=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(n + 3):
        if i >= 3:
            ev[i - 3][0].record()
        fn()
        if i >= 3:
            ev[i - 3][1].record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)[n // 2]


def synthetic_lm(order, n_total=1_000_000, seed=0):
    """A model of `order` over the token strings "0" .. str(V-1), ~n_total n-grams spread evenly over the orders >= 2: a k-gram
    is a random listed (k-1)-gram followed by a random word (the closure the reader demands), arbitrary values."""
    rng = np.random.default_rng(seed)
    vocab = ["<s>", "</s>", "<unk>"] + [str(t) for t in range(V)]
    W = len(vocab)
    per = n_total // (order - 1)
    grams = [np.arange(W, dtype=np.int32).reshape(-1, 1)]
    for k in range(2, order + 1):
        pre = grams[-1][grams[-1][:, -1] != 1]                      # nothing follows </s>
        g = np.concatenate([pre[rng.integers(0, len(pre), per)], rng.integers(1, W, (per, 1)).astype(np.int32)], 1)
        grams.append(np.unique(g, axis=0))
    orders = []
    for k, g in enumerate(grams, 1):
        lp = rng.uniform(-6, -0.05, len(g)).astype(np.float32)
        bo = rng.uniform(-2, 0.4, len(g)).astype(np.float32) if k < order else np.zeros(len(g), np.float32)
        orders.append((g, lp, bo, np.zeros(len(g), np.int64)))
    return NgramLM.from_arrays(vocab, orders, [str(t) for t in range(V)])


def main():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(B, T, V, generator=g) * 3.0
    logits[:, :, 0] += 3.0
    top_p, top_i = ops.topk_rows(logits.to(DEV), BEAM, log_softmax=True)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ws = torch.zeros(hip.lib().oe_ctc_prefix_beam_workspace_bytes(B, T, BEAM) // 4, dtype=torch.int32, device=DEV)
    pre = torch.zeros(B, BEAM, T, dtype=torch.int32, device=DEV)
    plen = torch.zeros(B, BEAM, dtype=torch.int32, device=DEV)
    total, ctc, lms = (torch.zeros(B, BEAM, dtype=torch.float64, device=DEV) for _ in range(3))

    plain_args = hip.prefix_beam_args(top_p, top_i, lens, BEAM, T, ws, pre, plen, ctc)

    def plain():
        hip.prefix_beam(plain_args)

    plain()
    print(f"top-k: {B} utterances x {T} frames, beam {BEAM}, V {V}; mean 1-best length {float(plen[:, 0].float().mean()):.1f} tokens")
    for order in (3, 5):
        lm = synthetic_lm(order)
        fused_args = hip.prefix_beam_args(top_p, top_i, lens, BEAM, T, ws, pre, plen, total, ctc, lms, lm=hip.ngram_model(lm, DEV),
                                          lm_weight=0.5, length_bonus=0.0, eos=True)
        print(f"model: order {lm.order}, {lm.n_ngrams} n-grams, table {lm.capacity} slots = {lm.capacity * 16 / 2 ** 20:.0f} MiB, "
              f"longest displacement {lm.max_probe}")

        def fused():
            hip.prefix_beam(fused_args)

        fused()
        torch.cuda.synchronize()
        assert int(ws[-1]) == 0
        best = pre[0, 0, : int(plen[0, 0])].tolist()
        host = lm.score(" ".join(str(t) for t in best))
        print(f"  utterance 0, fused 1-best of {len(best)} tokens: LM on the device {float(lms[0, 0]):.6f}, on the host {host:.6f}")
        runs = {"plain": [], "fused": []}
        for _ in range(3):
            runs["plain"].append(timed(plain))
            runs["fused"].append(timed(fused))
        a, b = sorted(runs["plain"])[1], sorted(runs["fused"])[1]
        for name, mid in (("plain", a), ("fused", b)):
            print(f"  {name}: {mid:8.1f} us per call = {mid / T:6.2f} us per frame (runs {', '.join('%.1f' % x for x in runs[name])})")
        print(f"  fused / plain: {b / a:.2f}")


if __name__ == "__main__":
    main()
