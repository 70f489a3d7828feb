#!/usr/bin/env python3
"""n-gram LM scoring on the device (oe_ngram_score) on its own and inside stage 2 of attention_rescoring_batch (GPU box).

  python tools/ngram_bench.py             # both parts
  python tools/ngram_bench.py --kernel    # (i)  oe_ngram_score alone: R = 640 hypotheses of ~35 and ~210 tokens, synthetic 3-gram model
                                          #      of ~1 M n-grams; half of every hypothesis walks listed 3-grams, half is random tokens
  python tools/ngram_bench.py --stage2    # (ii) stage 2 (bi-decoder pass + score mix) at bench.py's decode shape (64 x 10 s, beam 10),
                                          #      lm=None against the n-gram LM, eager and replayed from a HIP graph

HIP events, median of 20 calls after 3 warm-up calls, three alternating runs (the machine is shared); the middle run is reported."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import hip, ops, planes  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402

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


def synthetic_lm(V, n2, n3, seed=0):
    """A 3-gram model over the token strings "0" .. str(V-1): n2 random 2-grams, n3 3-grams that extend random listed 2-grams,
    arbitrary values - built from arrays (writing and parsing a million-line file would only time Python)."""
    rng = np.random.default_rng(seed)
    vocab = ["<s>", "</s>", "<unk>"] + [str(t) for t in range(V)]
    W = len(vocab)

    def vals(n):
        return rng.uniform(-6, -0.05, n).astype(np.float32), rng.uniform(-2, 0.4, n).astype(np.float32)

    g1 = np.arange(W, dtype=np.int32).reshape(-1, 1)
    g2 = np.unique(np.stack([rng.integers(2, W, n2), rng.integers(1, W, n2)], 1).astype(np.int32), axis=0)
    g2 = np.concatenate([g2, np.stack([np.zeros(V, np.int32), np.arange(3, W, dtype=np.int32)], 1)])       # <s> w
    pre = g2[g2[:, 1] != 1]                                                                                # nothing follows </s>
    g3 = np.unique(np.concatenate([pre[rng.integers(0, len(pre), n3)], rng.integers(1, W, (n3, 1)).astype(np.int32)], 1), axis=0)
    orders = []
    for g in (g1, g2, g3):
        lp, bo = vals(len(g))
        orders.append((g, lp, bo if g.shape[1] < 3 else np.zeros(len(g), np.float32), np.zeros(len(g), np.int64)))
    return NgramLM.from_arrays(vocab, orders, [str(t) for t in range(V)]), g3


def kernel_part():
    V = 3246
    lm, g3 = synthetic_lm(V, 330_000, 700_000)
    lm.to(DEV)
    print(f"model: order {lm.order}, {lm.n_ngrams} n-grams, table {lm.capacity} slots = {lm.capacity * 16 / 2 ** 20:.0f} MiB, "
          f"longest displacement {lm.max_probe}")
    rng = np.random.default_rng(1)
    R = 640
    for mean_len in (35, 210):
        ld = mean_len + 40
        lens = rng.integers(mean_len - 10, mean_len + 11, R).astype(np.int32)
        tokens = rng.integers(0, V, (R, ld)).astype(np.int32)
        walk = g3[rng.integers(0, len(g3), (R, ld // 6 + 1))].reshape(R, -1)[:, : ld // 2] - 3      # word id -> token id (may be < 0: <unk>)
        tokens[:, : walk.shape[1]] = np.clip(walk, 0, V - 1)
        tk, ln = torch.from_numpy(tokens).to(DEV), torch.from_numpy(lens).to(DEV)
        model = hip.ngram_model(lm, DEV)
        score = torch.empty(R, dtype=torch.float64, device=DEV)
        order = torch.zeros(R, ld + 1, dtype=torch.int32, device=DEV)
        lp = torch.zeros(R, ld + 1, dtype=torch.float64, device=DEV)

        def call(per_token=False):
            hip.call("oe_ngram_score", model, tk, ld, ln, R, 1, 1, score, lp if per_token else None, order if per_token else None)

        call(True)
        hist = torch.bincount(order[order > 0].flatten(), minlength=4).tolist()[1:]
        runs = [timed(call) for _ in range(3)]
        check = lm.score(" ".join(str(t) for t in tokens[0, : lens[0]]))
        print(f"oe_ngram_score R={R} x ~{mean_len} tokens: {sorted(runs)[1]:7.1f} us per call (runs {', '.join('%.1f' % x for x in runs)}); "
              f"matches by order 1/2/3: {hist}; row 0 device {float(score[0]):.6f} host {check:.6f}")


def stage2_part():
    from bench import MODEL_CONF, V
    from openeat_amd.models.asr_model import ASRModel
    from openeat_amd.utils import common
    hip.GEMM_PRECISION = int(os.environ.get("OE_GEMM_PRECISION", "6"))
    ops.PARALLEL_DECODERS = ops.POS_PROJ_AHEAD = False              # as bench.py's decode_rtf: one stream
    torch.manual_seed(4)
    model = ASRModel(80, V, **MODEL_CONF).to(DEV).eval()
    lm, _ = synthetic_lm(V, 330_000, 700_000)
    lm.to(DEV)
    B, beam = 64, 10
    torch.manual_seed(5)
    feats = torch.randn(B, 998, 80, device=DEV)
    flen = torch.full((B,), 998, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        enc, mask, pre, plen, ctc, bad, _ = model._rescore_stage1(feats, flen, hip.PrefixSearch(beam))
        Lm = max(int(plen.max()), 1)
        Lb = min(-(-Lm // 16) * 16, pre.shape[1])
        print(f"stage 2 at B={B} x 998 frames, beam {beam}: T'={enc.shape[1]}, R={B * beam}, longest hypothesis {Lm} (width {Lb}), "
              f"mean {float(plen.clamp(min=0).float().mean()):.1f} tokens")
        common.STATIC_SHAPES = True                                  # as _rescoring_batch_graphs: nothing reads a length on the host

        def stage2(which, w):
            return lambda: model._rescore_stage2(enc, mask, pre, plen, ctc, Lb, beam, 0.5, 0.3, which, w)

        variants = {"lm=None": stage2(None, 0.0), "n-gram LM": stage2(lm, 0.3)}
        picks = {k: f()[0].clone() for k, f in variants.items()}
        print(f"picks that differ between the two: {int((picks['lm=None'] != picks['n-gram LM']).any(1).sum())} of {B}")
        eager = {k: [] for k in variants}
        for _ in range(3):
            for k, f in variants.items():
                eager[k].append(timed(f))
        graphs, replay = {}, {k: [] for k in variants}
        for k, f in variants.items():
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with planes.capture_scope(), torch.cuda.graph(g):
                f()
            graphs[k] = g
        for _ in range(3):
            for k, g in graphs.items():
                replay[k].append(timed(g.replay))
    for name, res in (("eager", eager), ("graph replay", replay)):
        a, b = sorted(res["lm=None"])[1], sorted(res["n-gram LM"])[1]
        print(f"stage 2 {name}: lm=None {a / 1e3:8.3f} ms (runs {', '.join('%.3f' % (x / 1e3) for x in res['lm=None'])}), n-gram LM {b / 1e3:8.3f} ms "
              f"(runs {', '.join('%.3f' % (x / 1e3) for x in res['n-gram LM'])}): +{(b - a):.0f} us = {100 * (b - a) / a:+.2f} %")


if __name__ == "__main__":
    args = sys.argv[1:]
    if not args or "--kernel" in args:
        kernel_part()
    if not args or "--stage2" in args:
        stage2_part()
