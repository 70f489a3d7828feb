#!/usr/bin/env python3
"""The resumable CTC prefix beam search (oe_ctc_prefix_beam_chunk) on an hour of frames against the one-shot search
(oe_ctc_prefix_beam) over the same top-k (GPU box).

  python tools/stream_beam_bench.py       # 2 recordings x 90 112 frames (one hour at 40 ms), beam 10, 352 chunks of 256 frames

The top-k comes from random logits over 4233 tokens (randn * 3, blank + 3: peaky frames with frequent blanks), made block by
block so that the (T', V) logits never exist.  Two numbers:
  total vs one-shot   the time of all chunks of a recording (HIP events around the whole sequence; no n-best is written before
                      the last chunk) against one call of the one-shot kernel;
  per-chunk growth    the mean time of a chunk over the first and over the last tenth of the recording (an event pair around
                      every chunk): equal if the stable-prefix commit keeps the tails short.
One warm-up run of each, then three alternating runs (the machine is shared); every run is printed, the middle one reported,
the spread is max - min over the three.  Only kernels are timed: states, outputs and workspaces are allocated once.  The
chunked result is compared with the one-shot one bit for bit before anything is timed."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip, ops  # noqa: E402

DEV = "cuda"
V, B, T, BEAM, CHUNK, BLOCK = 4233, 2, 352 * 256, 10, 256, 4096


def topk():
    g = torch.Generator(device=DEV).manual_seed(13)
    ps, ix = [], []
    for a in range(0, T, BLOCK):
        logits = torch.randn(B, min(BLOCK, T - a), V, generator=g, device=DEV) * 3.0
        logits[:, :, 0] += 3.0
        p, i = ops.topk_rows(logits, BEAM, log_softmax=True)
        ps.append(p)
        ix.append(i)
    return torch.cat(ps, 1).contiguous(), torch.cat(ix, 1).contiguous()


def main():
    lib = hip.lib()
    top_p, top_i = topk()
    new = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=DEV)
    # one-shot
    ws1, pre1, plen1, score1 = new(lib.oe_ctc_prefix_beam_workspace_bytes(B, T, BEAM) // 4), new(B, BEAM, T), new(B, BEAM), new(B, BEAM, dtype=torch.float64)
    one_args = hip.prefix_beam_args(top_p, top_i, None, BEAM, T, ws1, pre1, plen1, score1)
    # chunked
    ws, pre, frm, plen, score = new(lib.oe_ctc_prefix_beam_workspace_bytes(B, CHUNK, BEAM) // 4), new(B, BEAM, T), new(B, BEAM, T), new(B, BEAM), \
        new(B, BEAM, dtype=torch.float64)
    states = [new(lib.oe_ctc_prefix_beam_state_bytes(B, BEAM, T), dtype=torch.uint8) for _ in range(2)]
    stable = [new(B, T), new(B, T), new(B)]
    starts = list(range(0, T, CHUNK))
    parts = [(top_p[:, a:a + CHUNK].contiguous(), top_i[:, a:a + CHUNK].contiguous()) for a in starts]
    args = [hip.prefix_beam_args(p, i, None, BEAM, T, ws, pre, plen, score) for p, i in parts]
    print(f"top-k: {B} recordings x {T} frames, beam {BEAM}, V {V}; {len(starts)} chunks of {CHUNK} frames; back-pointers "
          f"{ws1.numel() * 4 / 2 ** 20:.1f} MiB one-shot, {ws.numel() * 4 / 2 ** 20:.2f} MiB chunked; a state {states[0].numel() / 2 ** 20:.1f} MiB")

    def one_shot():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hip.prefix_beam(one_args)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def chunked():
        """-> (ms in all, [ms of every chunk])"""
        stable[2].zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(args) + 1)]
        cur = None
        ev[0].record()
        for k, a in enumerate(args):
            last = k == len(args) - 1
            hip.prefix_beam_chunk(a, cur, states[k & 1], *stable, frm, last=last, emit=False)
            cur = states[k & 1]
            ev[k + 1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[-1]), [x.elapsed_time(y) for x, y in zip(ev, ev[1:])]

    one_shot()
    chunked()
    assert int(ws1[-1]) == 0 and int(ws[-1]) == 0
    n = plen1[:, 0].tolist()
    same = torch.equal(plen, plen1) and torch.equal(score.view(torch.int64), score1.view(torch.int64)) and \
        all(torch.equal(pre[b, 0, : n[b]], pre1[b, 0, : n[b]]) for b in range(B))
    print(f"1-best lengths {n} tokens, stable at the end {stable[2].tolist()}; chunked == one-shot bit for bit: {same}")
    assert same
    runs = {"one": [], "all": [], "first": [], "last": []}
    tenth = max(len(args) // 10, 1)
    for _ in range(3):
        runs["one"].append(one_shot())
        ms, per = chunked()
        runs["all"].append(ms)
        runs["first"].append(sum(per[:tenth]) / tenth)
        runs["last"].append(sum(per[-tenth - 1:-1]) / tenth)                   # without the last chunk: it also writes the n-best
    mid = {k: sorted(v)[1] for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    fmt = lambda v: ", ".join("%.3f" % x for x in v)
    print(f"one-shot: {mid['one']:9.2f} ms = {mid['one'] * 1e3 / T:5.2f} us per frame (runs {fmt(runs['one'])})")
    print(f"chunked:  {mid['all']:9.2f} ms = {mid['all'] * 1e3 / T:5.2f} us per frame (runs {fmt(runs['all'])})")
    print(f"chunked / one-shot: {mid['all'] / mid['one']:.3f}")
    print(f"a chunk, first tenth: {mid['first']:.3f} ms (runs {fmt(runs['first'])}; spread {spread['first']:.3f})")
    print(f"a chunk, last tenth:  {mid['last']:.3f} ms (runs {fmt(runs['last'])}; spread {spread['last']:.3f})")
    grow = mid["last"] - mid["first"]
    print(f"last - first: {grow:+.3f} ms; the larger spread is {max(spread['first'], spread['last']):.3f} ms: "
          + ("no growth beyond the spread" if grow <= max(spread["first"], spread["last"]) else "the chunks GROW with the recording"))


if __name__ == "__main__":
    main()
