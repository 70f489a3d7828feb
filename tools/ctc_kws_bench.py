#!/usr/bin/env python3
"""Keyword search over CTC posteriors on the device (oe_ctc_kws) at the sizes of its users (GPU box).

  python tools/ctc_kws_bench.py [--out FILE]

Two shapes, V = 4233, K = 1000 keywords of 2 - 6 random labels, threshold confidence 0.5, max_hits 8:
  hour   one recording of T = 90 000 encoder frames (an hour of audio at 40 ms a frame)
  batch  B = 32 utterances of T = 250 frames
Synthetic logits: randn with +14 on planted occurrences of some keywords (each label one frame), so the call is also checked
at the size it is timed at: every planted occurrence must come back as a hit with its span.

The two launches are timed separately with HIP events alone: the call with every klens set to 0 is launch 1 (launch 2 then
only writes empty results), and the full call minus that is launch 2.  Median of 5 calls after 1 warm-up call, three runs (the
machine is shared), the middle one reported.  Launch 1's bytes are what the algorithm needs - the logits read once, the compact
rows written once - and are printed as bytes/s beside the HBM figures of the microarchitecture guide.  One JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.keyword import KeywordList  # noqa: E402

DEV = "cuda"
V, K, MAX_HITS = 4233, 1000, 8
HBM_ACHIEVABLE, HBM_SPEC = 6.3e12, 8.0e12            # bytes/s: measured float4 copy / data sheet


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


def middle(fn, **kw):
    runs = [timed(fn, **kw) for _ in range(3)]
    return sorted(runs)[1], [round(x, 3) for x in runs]


def keywords(seed):
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < K:
        y = tuple(int(c) for c in 1 + np.cumsum(rng.integers(1, V - 1, size=int(rng.integers(2, 7)))) % (V - 1))
        if y not in seen:                               # never the same label twice in a row
            seen.add(y)
            out.append(y)
    return KeywordList(out, threshold=0.5)


def planted(B, T, kl, seed, every):
    """-> logits (B, T, V) on the device and [(b, keyword, first frame, last frame)]: an occurrence about every `every` frames."""
    rng = np.random.default_rng(seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    logits = torch.randn(B, T, V, device=DEV, generator=g)
    where, bb, tt, cc = [], [], [], []
    for b in range(B):
        t = int(rng.integers(1, every))
        while t + 8 < T:
            k = int(rng.integers(0, K))
            y = kl.phrases[k]
            where.append((b, k, t, t + len(y) - 1))
            bb += [b] * len(y)
            tt += list(range(t, t + len(y)))
            cc += list(y)
            t += len(y) + int(rng.integers(every // 2, every))
    logits[torch.tensor(bb, device=DEV), torch.tensor(tt, device=DEV), torch.tensor(cc, device=DEV)] += 14.0
    return logits, where


def part(name, B, T, every):
    kl = keywords(7)
    U = len(kl.cols)
    logits, where = planted(B, T, kl, 11 + B, every)
    lib = hip.lib()
    nbytes = lib.oe_ctc_kws_workspace_bytes(B, T, U)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    n_hits = torch.empty(B, K, dtype=torch.int32, device=DEV)
    hs, he = (torch.empty(B, K, MAX_HITS, dtype=torch.int32, device=DEV) for _ in range(2))
    hv = torch.empty(B, K, MAX_HITS, device=DEV)
    bs, be = (torch.empty(B, K, dtype=torch.int32, device=DEV) for _ in range(2))
    bv = torch.empty(B, K, device=DEV)
    full = hip.keyword_set(kl, DEV)
    none = hip.keyword_set(kl, DEV)
    zero = torch.zeros(K, dtype=torch.int32, device=DEV)
    none.klens = zero.data_ptr()
    a = hip.CtcKwsArgs()
    a.logits, a.ldv, a.B, a.T, a.V, a.hlens = logits.data_ptr(), V, B, T, V, hl.data_ptr()
    a.normalized, a.max_hits, a.workspace = 0, MAX_HITS, ws.data_ptr()
    a.n_hits, a.hit_start, a.hit_end, a.hit_score = n_hits.data_ptr(), hs.data_ptr(), he.data_ptr(), hv.data_ptr()
    a.best_start, a.best_end, a.best_score = bs.data_ptr(), be.data_ptr(), bv.data_ptr()

    def call(q):
        a.kws = C.pointer(q)
        hip.check(lib.oe_ctc_kws(C.byref(a), hip.stream()), "oe_ctc_kws")

    call(full)
    torch.cuda.synchronize()
    n, s, e = n_hits.cpu().numpy(), hs.cpu().numpy(), he.cpu().numpy()
    assert n.max() <= MAX_HITS, "more hits than slots: the check below needs them all"
    got = {(b, k, int(s[b, k, i]), int(e[b, k, i])) for b, k in zip(*np.nonzero(n)) for i in range(n[b, k])}
    missing = [w for w in where if w not in got]
    assert not missing, f"{len(missing)} of {len(where)} planted occurrences did not come back: {missing[:5]}"
    reps = dict(n=5, warm=1) if B * T > 50000 else dict(n=20, warm=3)
    ms_rows, runs_rows = middle(lambda: call(none), **reps)
    ms_all, runs_all = middle(lambda: call(full), **reps)
    rows_bytes = B * T * (V + U + 1) * 4
    lens = np.asarray([len(p) for p in kl.phrases])
    return {"shape": name, "B": B, "T": T, "V": V, "K": K, "U": U, "labels": [int(lens.min()), int(lens.max())],
            "planted": len(where), "hits": int(n.sum()), "workspace_MiB": round(nbytes / 2 ** 20, 1),
            "call_ms": round(ms_all, 3), "call_runs_ms": runs_all,
            "launch1_ms": round(ms_rows, 3), "launch1_runs_ms": runs_rows, "launch1_bytes": rows_bytes,
            "launch1_TB_per_s": round(rows_bytes / ms_rows * 1e3 / 1e12, 3),
            "hbm_achievable_TB_per_s": HBM_ACHIEVABLE / 1e12, "hbm_spec_TB_per_s": HBM_SPEC / 1e12,
            "launch1_share_of_achievable": round(rows_bytes / ms_rows * 1e3 / HBM_ACHIEVABLE, 3),
            "launch2_ms": round(ms_all - ms_rows, 3), "launch2_ns_per_frame_of_a_wave": round((ms_all - ms_rows) * 1e6 / T, 1),
            "keyword_frames_per_s": round(B * K * T / (ms_all - ms_rows) * 1e3)}


if __name__ == "__main__":
    assert torch.cuda.is_available(), "ctc_kws_bench needs a GPU"
    res = {"bench": "ctc_kws", "device": torch.cuda.get_device_name(0),
           "shapes": [part("one hour of audio", 1, 90000, 600), part("one batch", 32, 250, 60)]}
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
