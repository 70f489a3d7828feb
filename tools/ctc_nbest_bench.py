#!/usr/bin/env python3
"""Grouped n-best CTC scoring (oe_ctc_nbest_score + oe_ctc_nbest_grad) against the expanded form it replaces (GPU box).

  python tools/ctc_nbest_bench.py           # the kernels: B = 32, T = 249, V = 3246 (rows padded to 3248), group = 10, hypotheses of 15-35
                                            # tokens that differ from their utterance's base sequence in one or two positions.
                                            # Baseline: what the library offered before - repeat_interleave of the logits (group-fold),
                                            # then oe_ctc_loss_fused with its gradient on B * group utterances, weighted by utt_weight
                                            # (the sum over the group that would still have to follow is NOT timed).
                                            # Prints one JSON line.
  python tools/ctc_nbest_bench.py --step    # a forward_mwer + backward step against a forward + backward step of the config-2 model
                                            # (12 + 3 + 3 blocks, d = 256) on 32 x 10 s of noise features: wall clock, one JSON line

HIP events, median of 20 calls after 3 warm-up calls, three runs (the machine is shared), the middle one reported.  Bytes are
algorithmic, in units of the logits' B*T*ldv*4: the grouped form reads them in the score, reads them and writes dlogits in
the grad (3 x); the baseline's copy reads 1 and writes `group`, its loss reads and writes `group` each (1 + 3 x group)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
HBM_PEAK = 8.0e12                  # bytes / s, the figure profiles/r04_ctc_bench.txt uses


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


def mid3(fn):
    runs = [timed(fn) for _ in range(3)]
    return sorted(runs)[1], runs


def kernel_part():
    B, T, V, ldv, group, Lmax = 32, 249, 3246, 3248, 10, 35
    R = B * group
    rng = np.random.default_rng(3)
    hyps = rng.integers(1, V, (R, Lmax)).astype(np.int32)
    lens = np.zeros(R, dtype=np.int32)
    for b in range(B):
        base = rng.integers(1, V, Lmax)
        for n in range(group):
            row = base.copy()
            for _ in range(1 + n % 2):
                row[rng.integers(0, 15)] = rng.integers(1, V)
            lens[b * group + n] = rng.integers(15, Lmax + 1)
            hyps[b * group + n] = row
    hlens = np.array([T - (b % 8) * 6 for b in range(B)], dtype=np.int32)
    logits = torch.randn(B, T, ldv, device=DEV) * 2.0
    hy, ln, hl = (torch.from_numpy(a).to(DEV) for a in (hyps, lens, hlens))
    g = torch.rand(R, device=DEV) * 2 - 1
    lib = hip.lib()
    ws = torch.empty(lib.oe_ctc_nbest_workspace_bytes(B, T, group, Lmax), dtype=torch.uint8, device=DEV)
    saved = torch.empty(lib.oe_ctc_nbest_saved_bytes(B, T, group, Lmax), dtype=torch.uint8, device=DEV)
    logp = torch.empty(R, device=DEV)
    dl = torch.empty(B, T, ldv, device=DEV)
    args = (logits, ldv, B, T, V, hl, hy, Lmax, ln, group, Lmax)

    def score(keep=True):
        hip.call("oe_ctc_nbest_score", *args, logp, saved if keep else None, ws)

    def grad():
        hip.call("oe_ctc_nbest_grad", *args, logp, g, saved, dl, None)

    def grouped():
        score()
        grad()

    # the expanded form
    ws_b = torch.empty(lib.oe_ctc_workspace_floats(R, T, Lmax), device=DEV)
    nll = torch.empty(R, device=DEV)
    tot = torch.empty(1, device=DEV)
    hl_r = hl.repeat_interleave(group)
    uw = -g

    def expanded():
        big = logits.repeat_interleave(group, 0)
        hip.call("oe_ctc_loss_fused", big, ldv, R, T, V, hl_r, hy, Lmax, ln, 1.0, uw, nll, tot, big, ws_b)
        return big

    grouped()
    big = expanded()
    torch.cuda.synchronize()
    # same numbers: logp = -nll, dlogits = the expanded gradient summed over the group
    d_logp = float((logp + nll).abs().max())
    d_grad = float((dl - big.view(B, group, T, ldv).sum(1))[..., :V].abs().max())
    del big
    t_score_only, _ = mid3(lambda: score(False))
    t_score, _ = mid3(score)
    t_grad, _ = mid3(grad)
    t_grouped, runs_g = mid3(grouped)
    t_expanded, runs_e = mid3(expanded)
    plane = B * T * ldv * 4
    out = {
        "bench": "ctc_nbest", "B": B, "T": T, "V": V, "ldv": ldv, "group": group, "hyp_len": [15, Lmax],
        "grouped_us": round(t_grouped, 1), "grouped_runs_us": [round(x, 1) for x in runs_g],
        "score_without_saved_us": round(t_score_only, 1), "score_us": round(t_score, 1), "grad_us": round(t_grad, 1),
        "grouped_bytes": 3 * plane, "grouped_fraction_of_hbm": round(3 * plane / (t_grouped * 1e-6) / HBM_PEAK, 4),
        "grad_bytes": 2 * plane, "grad_fraction_of_hbm": round(2 * plane / (t_grad * 1e-6) / HBM_PEAK, 4),
        "expanded_us": round(t_expanded, 1), "expanded_runs_us": [round(x, 1) for x in runs_e],
        "expanded_bytes": (1 + 3 * group) * plane, "expanded_fraction_of_hbm": round((1 + 3 * group) * plane / (t_expanded * 1e-6) / HBM_PEAK, 4),
        "ratio": round(t_expanded / t_grouped, 2), "max_abs_diff_logp": d_logp, "max_abs_diff_dlogits": d_grad,
    }
    print(json.dumps(out))


def step_part():
    from openeat_amd.models.asr_model import ASRModel
    V, B = 3246, 32
    torch.manual_seed(7)
    model = ASRModel(80, V, encoder_num_blocks=12, decoder_num_blocks=3, r_decoder_num_blocks=3, d_model=256, attention_heads=4,
                     linear_units=1024, dropout_rate=0.0, cnn_module_kernel=15, ctc_weight=0.3, reverse_weight=0.3).to(DEV).train()
    g = torch.Generator().manual_seed(8)
    feats = torch.randn(B, 998, 80, generator=g).to(DEV)
    nfr = torch.full((B,), 998, dtype=torch.int32, device=DEV)
    tl = torch.tensor([30 - b % 12 for b in range(B)], dtype=torch.int32)
    tgt = torch.randint(2, V - 1, (B, 30), generator=g, dtype=torch.int32).masked_fill(torch.arange(30).unsqueeze(0) >= tl.unsqueeze(1), -1)
    tgt, tl = tgt.to(DEV), tl.to(DEV)

    def run(mwer, n=8):
        ts = []
        for k in range(n + 2):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = model.forward_mwer(feats, nfr, tgt, tl, nbest=10)[0] if mwer else model(feats, nfr, tgt, tl)[0]
            loss.backward()
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    a, b = [], []
    for _ in range(3):
        a.append(run(False))
        b.append(run(True))
    fa, fb = sorted(a)[1], sorted(b)[1]
    print(json.dumps({"bench": "forward_mwer_step", "B": B, "frames": 998, "nbest": 10, "forward_ms": round(fa, 2),
                      "forward_mwer_ms": round(fb, 2), "ratio": round(fb / fa, 3), "forward_runs_ms": [round(x, 2) for x in a],
                      "forward_mwer_runs_ms": [round(x, 2) for x in b]}))


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        step_part()
    else:
        kernel_part()
