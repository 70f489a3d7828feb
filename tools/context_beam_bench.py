#!/usr/bin/env python3
"""The hotword-biased CTC prefix beam search (oe_ctc_prefix_beam with a context graph) against the plain and the LM-fused one
on the same top-k: the four instantiations of beam.hip's kernel (GPU box).

  python tools/context_beam_bench.py      # 64 utterances x 10 s (250 frames), beam 10; graphs of 0, 100 and 1000 phrases

Top-k and LM are those of tools/lm_beam_bench.py (random peaky logits over 3246 tokens; a synthetic order-3 model of ~1 M
n-grams).  The phrases are sub-sequences of 2..6 tokens of the plain search's own n-best lists, so they fire and their
prefixes are met all the time; c = 3.  Only the kernels are timed: outputs and workspace are allocated once.  HIP events,
median of 20 calls after 3 warm-up calls, three alternating runs (the machine is shared); the middle run is reported in
microseconds per call.  Prints the table and, last, one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lm_beam_bench import B, BEAM, T, V, synthetic_lm, timed  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.utils.context_graph import ContextGraph  # noqa: E402

DEV = "cuda"
SIZES = (0, 100, 1000)


def draw_phrases(nbest, n, rng):
    """n distinct sub-sequences of 2..6 tokens of the prefixes in `nbest`."""
    out = set()
    pool = [p for p in nbest if len(p) >= 2]
    for _ in range(200 * n):                                       # bounded: a short n-best may hold fewer than n sub-sequences
        if len(out) >= n:
            break
        p = pool[int(rng.integers(0, len(pool)))]
        k = int(rng.integers(2, min(6, len(p)) + 1))
        i = int(rng.integers(0, len(p) - k + 1))
        out.add(tuple(p[i:i + k]))
    return sorted(out)


def main():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(B, T, V, generator=g) * 3.0
    logits[:, :, 0] += 3.0
    top_p, top_i = ops.topk_rows(logits.to(DEV), BEAM, log_softmax=True)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ws = torch.zeros(hip.lib().oe_ctc_prefix_beam_workspace_bytes(B, T, BEAM) // 4, dtype=torch.int32, device=DEV)
    pre = torch.zeros(B, BEAM, T, dtype=torch.int32, device=DEV)
    plen = torch.zeros(B, BEAM, dtype=torch.int32, device=DEV)
    total, ctc, lms, bias = (torch.zeros(B, BEAM, dtype=torch.float64, device=DEV) for _ in range(4))
    lm = synthetic_lm(3)
    model = hip.ngram_model(lm, DEV)

    def search(*outs, **kw):
        a = hip.prefix_beam_args(top_p, top_i, lens, BEAM, T, ws, pre, plen, *outs, **kw)
        return lambda: hip.prefix_beam(a)

    plain = search(ctc)
    fused = search(total, ctc, lms, lm=model, lm_weight=0.5)

    def biased(graph, with_lm):
        return search(total, ctc, lms if with_lm else None, bias, lm=model if with_lm else None, ctx=hip.context_graph(graph, DEV),
                      lm_weight=0.5)

    plain()
    torch.cuda.synchronize()
    nbest = [tuple(pre[b, i, : int(plen[b, i])].tolist()) for b in range(B) for i in range(BEAM) if int(plen[b, i]) >= 0]
    rng = np.random.default_rng(7)
    fns = {"plain": plain, "lm": fused}
    info = {}
    for n in SIZES:
        graph = ContextGraph(draw_phrases(nbest, n, rng) if n else [], 3.0)
        info[n] = dict(phrases=len(graph.phrases), states=graph.n_states, capacity=graph.capacity, max_probe=graph.max_probe)
        for with_lm in (False, True):
            fns[f"ctx{n}" + ("+lm" if with_lm else "")] = biased(graph, with_lm)
    for name, fn in fns.items():                                   # every variant once, checked, before anything is timed
        fn()
        torch.cuda.synchronize()
        assert int(ws[-1]) == 0, name
        if name.startswith("ctx"):
            print(f"{name}: mean 1-best length {float(plen[:, 0].float().mean()):.1f} tokens, mean 1-best bias {float(bias[:, 0].mean()):.2f}")
    runs = {name: [] for name in fns}
    for _ in range(3):
        for name, fn in fns.items():
            runs[name].append(timed(fn))
    mid = {name: sorted(r)[1] for name, r in runs.items()}
    for name in fns:
        base = mid["lm"] if name.endswith("+lm") else mid["plain"]
        print(f"  {name:>10}: {mid[name]:8.1f} us per call = {mid[name] / T:6.2f} us per frame, x{mid[name] / base:.2f} of "
              f"{'lm' if name.endswith('+lm') else 'plain'} (runs {', '.join('%.1f' % x for x in runs[name])})")
    print(json.dumps({"tool": "context_beam_bench", "utterances": B, "frames": T, "beam": BEAM, "lm_order": lm.order,
                      "lm_ngrams": int(lm.n_ngrams), "graphs": {str(n): info[n] for n in SIZES},
                      "us_per_call": {k: round(v, 1) for k, v in mid.items()},
                      "runs_us": {k: [round(x, 1) for x in v] for k, v in runs.items()}}))


if __name__ == "__main__":
    main()
