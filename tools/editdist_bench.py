#!/usr/bin/env python3
"""Edit distance on the device (oe_edit_distance) on its own and inside Executor.cv (GPU box).

  python tools/editdist_bench.py            # both parts
  python tools/editdist_bench.py --kernel   # (i)  oe_edit_distance alone: 640 pairs (64 references x 10 hypotheses, group = 10) of ~35 and
                                            #      ~210 tokens, every hypothesis its reference with ~10 % of the tokens replaced, dropped
                                            #      or doubled; counts only and with the alignment
  python tools/editdist_bench.py --cv       # (ii) Executor.cv on the tiny conformer the test suite uses (2 + 1 blocks, d_model 32), two
                                            #      batches of three utterances of up to 95 frames, with cv_error_rate off and on

(i) HIP events, median of 20 calls after 3 warm-up calls, three runs (the machine is shared), the middle one reported;
(ii) wall clock around cv (it reads the loss back every batch), median of 20 after 3 warm-up calls, three alternating runs."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip  # noqa: E402

DEV = "cuda"


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


def kernel_part():
    V, U, beam = 3246, 64, 10
    P = U * beam
    rng = np.random.default_rng(1)
    for mean_len in (35, 210):
        Nmax = Mmax = mean_len + 40
        ref = rng.integers(1, V, (U, Nmax)).astype(np.int32)
        rl = rng.integers(mean_len - 10, mean_len + 11, U).astype(np.int32)
        hyp = np.zeros((P, Mmax), dtype=np.int32)
        hl = np.zeros(P, dtype=np.int32)
        for p in range(P):
            out = []
            for t in ref[p // beam, : rl[p // beam]]:
                x = rng.random()
                if x < 0.03:
                    continue
                out.append(int(rng.integers(1, V)) if x < 0.07 else int(t))
                if x > 0.97:
                    out.append(int(t))
            out = out[:Mmax]
            hyp[p, : len(out)], hl[p] = out, len(out)
        ref_d, rl_d, hyp_d, hl_d = (torch.from_numpy(a).to(DEV) for a in (ref, rl, hyp, hl))
        counts = torch.empty(P, 4, dtype=torch.int32, device=DEV)
        r2h = torch.empty(P, Nmax, dtype=torch.int32, device=DEV)
        nbytes = hip.lib().oe_edit_distance_workspace_bytes(P, Nmax, Mmax)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None

        def call(align):
            hip.call("oe_edit_distance", ref_d, Nmax, rl_d, beam, hyp_d, Mmax, hl_d, P, Nmax, Mmax, counts, r2h if align else None, ws)

        call(True)
        c = counts.sum(0).tolist()
        only = [timed(lambda: call(False)) for _ in range(3)]
        full = [timed(lambda: call(True)) for _ in range(3)]
        print(f"oe_edit_distance P={P} x ~{mean_len} tokens (Nmax = Mmax = {Nmax}, back-pointers in {'the workspace' if nbytes else 'LDS'}): "
              f"counts only {sorted(only)[1]:7.1f} us (runs {', '.join('%.1f' % x for x in only)}), aligned {sorted(full)[1]:7.1f} us "
              f"(runs {', '.join('%.1f' % x for x in full)}); C/S/D/I = {c}, error rate {100.0 * sum(c[1:]) / sum(c[:3]):.2f} %")


def cv_part():
    from openeat_amd.models.asr_model import ASRModel
    from openeat_amd.utils.executor import Executor
    torch.manual_seed(7)
    model = ASRModel(80, 40, encoder_num_blocks=2, decoder_num_blocks=1, r_decoder_num_blocks=1, d_model=32, attention_heads=4,
                     linear_units=64, reverse_weight=0.3, dropout_rate=0.0).to(DEV).eval()
    feats = torch.randn(3, 95, 80)
    tlen = torch.tensor([7, 5, 3])
    tgt = torch.randint(1, 39, (3, 7)).masked_fill(torch.arange(7).unsqueeze(0) >= tlen.unsqueeze(1), -1)
    batch = {"features": feats, "features_length": torch.tensor([95, 70, 43], dtype=torch.int32), "targets": tgt, "targets_length": tlen}
    loader = [(["a", "b", "c"], batch), (["d", "e", "f"], batch)]

    class Quiet:
        def info(self, msg):
            self.last = msg

    log, ex = Quiet(), Executor()

    def run(flag, n=20):
        ts = []
        for k in range(n + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex.cv(log, model, loader, torch.device(DEV), {"log_interval": 1000, "cv_error_rate": flag})
            torch.cuda.synchronize()
            if k >= 3:
                ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[n // 2]

    off, on = [], []
    for _ in range(3):
        off.append(run(False))
        on.append(run(True))
    a, b = sorted(off)[1], sorted(on)[1]
    print(f"Executor.cv, tiny conformer, 2 batches x 3 utterances of {tuple(feats.shape[1:])} features: cv_error_rate off {a:7.3f} ms "
          f"(runs {', '.join('%.3f' % x for x in off)}), on {b:7.3f} ms (runs {', '.join('%.3f' % x for x in on)}): +{b - a:.3f} ms = "
          f"{100 * (b - a) / a:+.1f} %; {log.last}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if not args or "--kernel" in args:
        kernel_part()
    if not args or "--cv" in args:
        cv_part()
