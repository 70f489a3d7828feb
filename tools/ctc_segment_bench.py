#!/usr/bin/env python3
"""Long-form CTC segmentation on the device (oe_ctc_segment) at the size of a 30-minute recording (GPU box).

  python tools/ctc_segment_bench.py [--out FILE]

T = 45 000 encoder frames, L = 7 000 labels (S = 14 001 states, 6.3e8 cells), V = 4233, B = 1 and B = 8 recordings; synthetic
logits: randn with +12 on a planted path (every label one frame, labels at random frames, blanks elsewhere), so the call is
also checked at the size it is timed at: `frames` must be the planted tokens.  For context, oe_ctc_align on the same 45 000
frames cut into 150 utterances of 300 frames and 47 labels (what a user had to do by hand before).

HIP events around the whole call (both launches), median of 5 calls after 1 warm-up call, three runs (the machine is shared), the
middle one reported.  Prints one JSON line: times in ms, and frames per second of the chain (B * T / time)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
T, L, V = 45000, 7000, 4233


def timed(fn, n=5, warm=1):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(n + warm):
        if i >= warm:
            ev[i - warm][0].record()
        fn()
        if i >= warm:
            ev[i - warm][1].record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[n // 2]


def planted(B, seed):
    """-> logits (B, T, V) on the device, ys (B, L) int32, the planted token of every frame (B, T) int32."""
    rng = np.random.default_rng(seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    logits = torch.randn(B, T, V, device=DEV, generator=g)
    ys = np.zeros((B, L), dtype=np.int32)
    tok = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ys[b] = 1 + np.cumsum(rng.integers(1, V - 1, size=L)) % (V - 1)          # never the same label twice in a row
        at = np.sort(rng.choice(np.arange(100, T - 100), size=L, replace=False))
        tok[b, at] = ys[b]
    tok_d = torch.from_numpy(tok).to(DEV)
    logits.scatter_add_(2, tok_d.long().unsqueeze(2), torch.full((B, T, 1), 12.0, device=DEV))
    return logits, torch.from_numpy(ys).to(DEV), tok_d


def segment_part(B):
    logits, ys, tok = planted(B, 90 + B)
    lib = hip.lib()
    hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    yl = torch.full((B,), L, dtype=torch.int32, device=DEV)
    nbytes = lib.oe_ctc_segment_workspace_bytes(B, T, V, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    frames = torch.empty(B, T, dtype=torch.int32, device=DEV)
    pl = torch.empty(B, T, device=DEV)
    st, en = (torch.empty(B, L, dtype=torch.int32, device=DEV) for _ in range(2))
    lg = torch.empty(B, L, device=DEV)
    score = torch.empty(B, dtype=torch.float64, device=DEV)
    a = hip.CtcSegmentArgs()
    a.logits, a.ldv, a.B, a.T, a.V = logits.data_ptr(), V, B, T, V
    a.hlens, a.targets, a.Lmax, a.tlens = hl.data_ptr(), ys.data_ptr(), L, yl.data_ptr()
    a.free_start, a.free_end = 1, 1
    a.frames, a.path_logp, a.tok_start, a.tok_end, a.tok_logp = frames.data_ptr(), pl.data_ptr(), st.data_ptr(), en.data_ptr(), lg.data_ptr()
    a.score, a.workspace = score.data_ptr(), ws.data_ptr()

    def call():
        hip.check(lib.oe_ctc_segment(C.byref(a), hip.stream()), "oe_ctc_segment")

    call()
    torch.cuda.synchronize()
    assert torch.equal(frames, tok), "the planted path did not come back"
    assert bool(torch.isfinite(score).all()) and bool((st == en).all())
    runs = [timed(call) for _ in range(3)]
    ms = sorted(runs)[1]
    return {"B": B, "ms": round(ms, 3), "runs_ms": [round(x, 3) for x in runs], "frames_per_s": round(B * T / ms * 1e3),
            "us_per_frame_of_one_recording": round(ms * 1e3 / T, 3), "workspace_MiB": round(nbytes / 2 ** 20, 1),
            "score": float(score[0])}


def align_part():
    """The same frames as 150 utterances of 300 frames and 47 labels through oe_ctc_align."""
    B, Tu, Lu = 150, 300, 47
    g = torch.Generator(device=DEV).manual_seed(99)
    logits = torch.randn(B, Tu, V, device=DEV, generator=g)
    ys = torch.randint(1, V, (B, Lu), dtype=torch.int32, device=DEV, generator=g)
    hl = torch.full((B,), Tu, dtype=torch.int32, device=DEV)
    yl = torch.full((B,), Lu, dtype=torch.int32, device=DEV)
    lib = hip.lib()
    ws = torch.empty(lib.oe_ctc_align_workspace_bytes(B, Tu, Lu), dtype=torch.uint8, device=DEV)
    frames = torch.empty(B, Tu, dtype=torch.int32, device=DEV)
    st, en = (torch.empty(B, Lu, dtype=torch.int32, device=DEV) for _ in range(2))
    lg = torch.empty(B, Lu, device=DEV)
    score = torch.empty(B, device=DEV)

    def call():
        hip.call("oe_ctc_align", logits, V, B, Tu, V, hl, ys, Lu, yl, frames, st, en, lg, score, ws)

    call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(score).all())
    runs = [timed(call, n=20, warm=3) for _ in range(3)]
    return {"utterances": B, "frames": Tu, "labels": Lu, "ms": round(sorted(runs)[1], 3), "runs_ms": [round(x, 3) for x in runs]}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_segment_bench needs a GPU"
    res = {"bench": "ctc_segment", "T": T, "L": L, "V": V, "cells": T * (2 * L + 1), "segment": [segment_part(1), segment_part(8)],
           "align_cut_by_hand": align_part()}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
