#!/usr/bin/env python3
"""The joint CTC/attention beam search at the decode leg's shape (GPU box): the CTC prefix-score kernel per step, the whole
search, and recognize at the same beam on the same batch.

  python tools/joint_search_bench.py                # 64 utterances x 10 s (249 encoder frames), beam 10, 20 candidates, V 3246
  python tools/joint_search_bench.py --lm-order 3   # also (iii) and the search with an n-gram LM of that order (0 = off)
  python tools/joint_search_bench.py --hotwords 1000  # also (iv) and the search with a context graph of that many phrases

(i)  oe_ctc_prefix_score alone, 640 hypotheses x 20 candidates x 249 frames, on hypotheses three tokens deep (their states come
     from the kernel itself), with and without the candidates' states.  The CTC log-probabilities are the log-softmax of random
     logits (randn * 3, blank + 3: peaky frames with frequent blanks, as a CTC posterior has them), the candidates the top-20 of
     random attention scores.  HIP events, median of 20 calls after 3 warm-up calls, three runs, the middle one reported.
(ii) ASRModel.ctc_attention_beam_search (ctc_weight 0.3, and 0: the same loop without the kernel) and ASRModel.recognize on
     bench.py's 12-layer Conformer with seeded random weights, random features, every call to its end on the host clock between
     two device synchronisations; one warm-up round, then three alternating rounds, the middle one reported.  An untrained
     decoder hardly ever emits <eos>, so all three run to the step limit, the encoder length: the same number of decoder steps.
(iii) --lm-order N: oe_ngram_next alone on 640 hypotheses twelve tokens deep - the full-vocabulary form (640 x 3246 terms) and
     the candidate form (640 x 20, the top-20 of random attention scores) - timed as (i), and in (ii) the search at ctc_weight 0.3
     with the LM at lm_weight 0.5, pre-selected with the LM (one full-vocabulary call per step) and without (one candidate call).
     The LM is synthetic and sized like an AISHELL character LM (tools/lm_beam_bench.py's: ~1 M n-grams over the 3246 tokens, a
     32 MiB table), its values arbitrary: the searches with it take other paths through the vocabulary, not fewer steps.
(iv) --hotwords N: oe_context_next alone on 640 hypotheses, half of them in the root and half in random states of the automaton
     - the candidate form (640 x 20, all three outputs) and the full-vocabulary form (640 x 3246, out_bias only) - timed as (i),
     and in (ii) the search at ctc_weight 0.3 with the graph, pre-selected with the bias (one full-vocabulary and one candidate
     call per step) and without (one candidate call); with --lm-order as well, the search with the LM and the graph together,
     both pre-selected.  The graph is synthetic: N distinct random phrases of 2..6 tokens over the 3246 tokens, context_score 3."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import ops  # noqa: E402
from openeat_amd.models.asr_model import ASRModel  # noqa: E402
from openeat_amd.utils import joint_search as js  # noqa: E402

DEV = "cuda"
V, B, SECONDS, BEAM, C = 3246, 64, 10, 10, 20
MODEL_CONF = dict(encoder_num_blocks=12, decoder_num_blocks=3, r_decoder_num_blocks=3, d_model=256, attention_heads=4,
                  linear_units=1024, dropout_rate=0.1, input_layer="conv2d", pos_enc_layer_type="rel_pos",
                  activation_type="swish", macaron_style=True, use_cnn_module=True, cnn_module_kernel=15, causal=False,
                  ctc_weight=0.3, lsm_weight=0.1, reverse_weight=0.3, length_normalized_loss=False)      # bench.py's


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


def kernel_leg(T):
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(B, T, V, generator=g) * 3.0
    logits[:, :, 0] += 3.0
    logp = ops.log_softmax_rows(logits.to(DEV))
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    R = B * BEAM
    att = ops.log_softmax_rows((torch.randn(4, R, V, generator=g) * 3.0).to(DEV))
    st = js.initial_state(logp, lens, BEAM, 0.3)
    for d in range(3):
        st = js.search_step(logp, lens, st, att[d], BEAM, C, V - 1, 0.3, 0.0)
    _, cand = ops.topk_rows(att[3], C)
    last = st.tokens[:, -1].contiguous()
    hyp_len = st.length.to(torch.int32)
    cand_state = torch.empty(R, T, C, 2, dtype=torch.float64, device=DEV)
    live = int(((st.total > -float("inf")) & ~st.finished).sum())
    print(f"(i) oe_ctc_prefix_score: {R} hypotheses ({live} live, {int(st.length.max())} tokens deep) x {C} candidates x {T} frames, V {V}")
    runs = {"with states": [], "psi only": []}
    for _ in range(3):
        runs["with states"].append(timed(lambda: ops.ctc_prefix_score(logp, lens, st.state, hyp_len, last, cand, V - 1, group=BEAM,
                                                                      cand_state=cand_state)))
        runs["psi only"].append(timed(lambda: ops.ctc_prefix_score(logp, lens, st.state, hyp_len, last, cand, V - 1, group=BEAM,
                                                                   states=False)))
    for name, r in runs.items():
        mid = sorted(r)[1]
        print(f"  {name}: {mid:8.1f} us per step = {mid * 1e3 / T:6.1f} ns per frame (runs {', '.join('%.1f' % x for x in r)})")
    print(f"  states written per step: {R * T * C * 16 / 2 ** 20:.1f} MiB")


def lm_leg(lm):
    g = torch.Generator().manual_seed(13)
    R, depth = B * BEAM, 12
    tokens = torch.randint(1, V - 1, (R, depth), generator=g).to(DEV)
    lens = torch.full((R,), depth, dtype=torch.int32, device=DEV)
    _, cand = ops.topk_rows(ops.log_softmax_rows((torch.randn(R, V, generator=g) * 3.0).to(DEV)), C)
    print(f"(iii) oe_ngram_next: order {lm.order}, {lm.n_ngrams} n-grams, table {lm.capacity * 16 / 2 ** 20:.0f} MiB, max_probe {lm.max_probe}; "
          f"{R} hypotheses {depth} tokens deep")
    runs = {f"every token ({V})": [], f"{C} candidates": []}
    for _ in range(3):
        runs[f"every token ({V})"].append(timed(lambda: ops.ngram_next(lm, tokens, lens, None, V - 1)))
        runs[f"{C} candidates"].append(timed(lambda: ops.ngram_next(lm, tokens, lens, cand, V - 1)))
    for (name, r), n in zip(runs.items(), (R * V, R * C)):
        mid = sorted(r)[1]
        print(f"  {name}: {mid:8.1f} us per call = {mid * 1e3 / n:6.2f} ns per term (runs {', '.join('%.1f' % x for x in r)})")


def synthetic_graph(n):
    from openeat_amd.utils.context_graph import ContextGraph
    g = torch.Generator().manual_seed(17)
    phrases = set()
    while len(phrases) < n:
        phrases.add(tuple(torch.randint(1, V - 1, (int(torch.randint(2, 7, (1,), generator=g)),), generator=g).tolist()))
    return ContextGraph(sorted(phrases), 3.0)


def context_leg(graph):
    g = torch.Generator().manual_seed(19)
    R = B * BEAM
    state = torch.randint(0, graph.n_states, (R,), generator=g, dtype=torch.int32)
    state[::2] = 0
    state = state.to(DEV)
    hits = (torch.rand(R, generator=g, dtype=torch.float64) * 9.0).to(DEV)
    _, cand = ops.topk_rows(ops.log_softmax_rows((torch.randn(R, V, generator=g) * 3.0).to(DEV)), C)
    print(f"(iv) oe_context_next: {len(graph.phrases)} phrases, {graph.n_states} states, edge table {graph.capacity * 16 / 2 ** 10:.0f} KiB, "
          f"max_probe {graph.max_probe}; {R} hypotheses, every second one in the root")
    runs = {f"{C} candidates": [], f"every token ({V})": []}
    for _ in range(3):
        runs[f"{C} candidates"].append(timed(lambda: ops.context_next(graph, state, hits, cand, V - 1)))
        runs[f"every token ({V})"].append(timed(lambda: ops.context_next(graph, state, hits, None, V - 1, V=V, want_state=False)))
    for (name, r), n in zip(runs.items(), (R * C, R * V)):
        mid = sorted(r)[1]
        print(f"  {name}: {mid:8.1f} us per call = {mid * 1e3 / n:6.2f} ns per entry (runs {', '.join('%.1f' % x for x in r)})")


def search_leg(lm=None, graph=None):
    torch.manual_seed(7)
    model = ASRModel(80, V, **MODEL_CONF).to(DEV).eval()
    g = torch.Generator().manual_seed(123)
    feats = torch.randn(B, SECONDS * 100 - 2, 80, generator=g).to(DEV)
    flen = torch.full((B,), feats.shape[1], dtype=torch.int32, device=DEV)
    out = {}

    def wall(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[name] = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    legs = {"joint search, ctc_weight 0.3": lambda: model.ctc_attention_beam_search(feats, flen, BEAM, 0.3, ctc_candidates=C),
            "joint search, ctc_weight 0  ": lambda: model.ctc_attention_beam_search(feats, flen, BEAM, 0.0, ctc_candidates=C),
            "recognize                   ": lambda: model.recognize(feats, flen, BEAM).tolist()}
    if lm is not None:
        for name, pre in (("joint search, 0.3 + LM, prebeam", True), ("joint search, 0.3 + LM, top-C  ", False)):
            legs[name] = lambda pre=pre: model.ctc_attention_beam_search(feats, flen, BEAM, 0.3, ctc_candidates=C, lm=lm, lm_weight=0.5,
                                                                         lm_prebeam=pre)
    if graph is not None:
        for name, pre in (("joint search, 0.3 + hotwords, prebeam", True), ("joint search, 0.3 + hotwords, top-C  ", False)):
            legs[name] = lambda pre=pre: model.ctc_attention_beam_search(feats, flen, BEAM, 0.3, ctc_candidates=C, context=graph,
                                                                         context_prebeam=pre)
        if lm is not None:
            legs["joint search, 0.3 + LM + hotwords, prebeam"] = lambda: model.ctc_attention_beam_search(
                feats, flen, BEAM, 0.3, ctc_candidates=C, lm=lm, lm_weight=0.5, lm_prebeam=True, context=graph, context_prebeam=True)
    runs = {k: [] for k in legs}
    with torch.no_grad():
        for it in range(4):
            for name, fn in legs.items():
                t = wall(name, fn)
                if it:
                    runs[name].append(t)
    steps = model._encode(feats, flen)[0].shape[1]
    print(f"(ii) {B} utterances x {SECONDS} s = {steps} encoder frames = decoder steps, beam {BEAM}, {C} candidates")
    mids = {}
    for name, r in runs.items():
        mids[name] = sorted(r)[1]
        mean_len = sum(len([t for t in h if t != V - 1]) for h in out[name]) / B
        print(f"  {name}: {mids[name] * 1e3:8.1f} ms = {mids[name] * 1e6 / steps:7.1f} us per step, mean output {mean_len:.1f} tokens "
              f"(runs {', '.join('%.1f' % (x * 1e3) for x in r)})")
    a, b, c = list(mids.values())[:3]
    for name in list(mids)[3:]:
        print(f"  {name.strip()} / joint (0.3): {mids[name] / a:.3f};  what it adds to a step: {(mids[name] - a) * 1e6 / steps:.1f} us")
    print(f"  joint (0.3) / recognize: {a / c:.2f};  joint (0) / recognize: {b / c:.2f};  the CTC side of a step: {(a - b) * 1e6 / steps:.1f} us")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lm-order", type=int, default=0, help="also time oe_ngram_next and the search with a synthetic n-gram LM of this order (2..5; 0: off)")
    ap.add_argument("--hotwords", type=int, default=0, help="also time oe_context_next and the search with a synthetic context graph of this many phrases (0: off)")
    args = ap.parse_args()
    if args.hotwords < 0:
        ap.error("--hotwords takes 0 or a number of phrases")
    if args.lm_order and not 2 <= args.lm_order <= 5:
        ap.error("--lm-order takes 0 or 2..5")
    lm = None
    if args.lm_order:
        from lm_beam_bench import synthetic_lm                      # beside this file
        lm = synthetic_lm(args.lm_order).to(DEV)
    kernel_leg(SECONDS * 25 - 1)
    if lm is not None:
        lm_leg(lm)
    graph = synthetic_graph(args.hotwords) if args.hotwords else None
    if graph is not None:
        context_leg(graph)
    search_leg(lm, graph)
