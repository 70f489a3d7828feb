#!/usr/bin/env python3
"""The transducer loss (oe_rnnt_loss + oe_rnnt_grad) launch by launch, and ops.rnnt_loss forward + backward (GPU box).

  python tools/rnnt_bench.py            # three shapes: B=4 T=100 U=15 V=512; B=8 T=250 U=30 V=4233 (1.05 GB of logits); B=4 T=500
                                        # U=60 V=4233.  Full lengths (every node inside its lattice: the most bytes a shape can
                                        # move).  One JSON line per shape.
  python tools/rnnt_bench.py --once     # the middle shape, the two calls three times each and nothing else: for a kernel trace,
                                        # which gives the row pass and the lattice pass of oe_rnnt_loss apart exactly

HIP events, median of 20 calls after 3 warm-up calls, three runs (the machine is shared), the middle one reported.
oe_rnnt_loss is two launches behind one call: `loss_us` times both; `lattice_us` is the same call on a V = 2 copy of the shape,
where the row pass reads 8 bytes a node and the lattice pass is unchanged (it never sees V); `rows_us` = loss_us - lattice_us.
Bytes are algorithmic.  With N = B*T*(U+1) nodes: the row pass reads the logits (4NV) and writes 12N; the lattice pass reads
8N and writes 16N; the gradient pass reads the logits and 36N of workspace and writes the logits' size (4NV), in place.  The
yardstick is oe_log_softmax over the same N rows: it reads 4NV and writes 4NV, as the gradient pass does."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip, ops  # noqa: E402

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
    return sorted(timed(fn) for _ in range(3))[1]


class Problem:
    def __init__(self, B, T, U, V, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.U, self.V = B, T, U, V
        self.logits = (torch.randn(B, T, U + 1, V, generator=g) * 2.0).to(DEV) if V > 2 else torch.zeros(B, T, U + 1, V, device=DEV)
        self.hl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        self.ul = torch.full((B,), U, dtype=torch.int32, device=DEV)
        self.tg = torch.randint(1, V, (B, max(U, 1)), generator=g, dtype=torch.int32).to(DEV)
        self.g = torch.ones(B, device=DEV)
        self.logp = torch.empty(B, device=DEV)
        self.ws = torch.empty(hip.lib().oe_rnnt_workspace_bytes(B, T, U), dtype=torch.uint8, device=DEV)

    def loss(self):
        a = hip.RnntArgs()
        a.logits, a.ldv, a.B, a.T, a.Umax, a.V = self.logits.data_ptr(), self.V, self.B, self.T, self.U, self.V
        a.hlens, a.targets, a.ulens = self.hl.data_ptr(), self.tg.data_ptr(), self.ul.data_ptr()
        a.blank, a.logp, a.status, a.workspace = 0, self.logp.data_ptr(), None, self.ws.data_ptr()
        hip.check(hip.lib().oe_rnnt_loss(hip.C.byref(a), hip.stream()), "oe_rnnt_loss")

    def grad(self, out):
        a = hip.RnntGradArgs()
        a.logits, a.ldv, a.B, a.T, a.Umax, a.V = self.logits.data_ptr(), self.V, self.B, self.T, self.U, self.V
        a.hlens, a.targets, a.ulens = self.hl.data_ptr(), self.tg.data_ptr(), self.ul.data_ptr()
        a.blank, a.g, a.dlogits, a.workspace = 0, self.g.data_ptr(), out.data_ptr(), self.ws.data_ptr()
        hip.check(hip.lib().oe_rnnt_grad(hip.C.byref(a), hip.stream()), "oe_rnnt_grad")


def shape(B, T, U, V):
    p = Problem(B, T, U, V)
    N = B * T * (U + 1)
    plane = 4 * N * V
    out = torch.empty_like(p.logits)
    p.loss()
    torch.cuda.synchronize()
    t_loss = mid3(p.loss)
    t_grad = mid3(lambda: p.grad(out))                 # out of place: the logits stay what the workspace was made from
    small = Problem(B, T, U, 2)
    t_lattice = mid3(small.loss)
    del small
    t_rows = t_loss - t_lattice
    t_lsm = mid3(lambda: hip.call("oe_log_softmax", p.logits, N, V, out))
    del out

    def op():                                          # out of place, so that the logits survive the call; in place moves the same bytes
        x = p.logits.detach().requires_grad_(True)
        ops.rnnt_loss(x, p.hl, p.tg[:, :U], p.ul).sum().backward()

    t_op = mid3(op)
    res = {
        "bench": "rnnt", "B": B, "T": T, "U": U, "V": V, "nodes": N, "logits_bytes": plane, "workspace_bytes": int(p.ws.numel()),
        "loss_us": round(t_loss, 1), "lattice_us": round(t_lattice, 1), "rows_us": round(t_rows, 1), "grad_us": round(t_grad, 1),
        "op_fwd_bwd_us": round(t_op, 1),
        "rows_bytes": plane + 12 * N, "rows_fraction_of_hbm": round((plane + 12 * N) / (t_rows * 1e-6) / HBM_PEAK, 4),
        "lattice_bytes": 24 * N,
        "grad_bytes": 2 * plane + 36 * N, "grad_fraction_of_hbm": round((2 * plane + 36 * N) / (t_grad * 1e-6) / HBM_PEAK, 4),
        "total_bytes": 3 * plane + 72 * N,
        "log_softmax_us": round(t_lsm, 1), "log_softmax_bytes": 2 * plane,
        "log_softmax_fraction_of_hbm": round(2 * plane / (t_lsm * 1e-6) / HBM_PEAK, 4),
        "grad_over_log_softmax": round(t_grad / t_lsm, 3), "rows_over_half_log_softmax": round(t_rows / (t_lsm / 2), 3),
    }
    print(json.dumps(res), flush=True)


def once():
    p = Problem(8, 250, 30, 4233)
    out = torch.empty_like(p.logits)
    for _ in range(3):
        p.loss()
        p.grad(out)
    hip.call("oe_log_softmax", p.logits, p.B * p.T * (p.U + 1), p.V, out)
    torch.cuda.synchronize()
    print("done")


if __name__ == "__main__":
    if "--once" in sys.argv[1:]:
        once()
    else:
        for s in ((4, 100, 15, 512), (8, 250, 30, 4233), (4, 500, 60, 4233)):
            shape(*s)
