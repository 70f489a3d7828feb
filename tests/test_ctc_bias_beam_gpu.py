"""GPU: CTC prefix beam search with hotword biasing on the device (oe_ctc_prefix_beam with a graph) against the yardstick
(tests/ctc_bias_beam_ref.py: the dict loop with the biased key, the bias by brute force from the definition - independent of
the product and held to what is pinned by tests/test_ctc_bias_beam_ref.py), run on the device's own top-k.

Bounds, those of tests/test_ctc_lm_beam_gpu.py: the same prefixes in the same order, exactly (the cases keep neighbouring
totals 1e-8 apart or exactly equal, asserted again on the top-k really used); total and ctc within 1e-9 * max(1, |x|); lm
within 2**-52 * n * S.  bias is EXACTLY equal: both sides add the same float32 values in float64 in the same order."""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_bias_beam_ref as BR  # noqa: E402
import ctc_lm_beam_ref as R  # noqa: E402
import ngram_ref  # noqa: E402
from test_ctc_lm_beam_gpu import _built_lm, _close, _model, _ragged  # noqa: E402
from openeat_amd.hip import PrefixSearch  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402
from openeat_amd.utils.context_graph import ContextGraph  # noqa: E402

DEV = "cuda"
GAP_FLOOR = 1e-8
NEG = -np.inf


def _device_graph(ref_graph):
    return ContextGraph(ref_graph[0], float(ref_graph[2]), ref_graph[1])


def _compare(got, want, ref, t2c, eos, where):
    """One utterance: device n-best [(prefix, total, ctc, lm, bias)] against the yardstick's; ref None: no LM."""
    assert [h[0] for h in got] == [h[0] for h in want], (where, got[:3], want[:3])
    for g, w in zip(got, want):
        assert _close(g[1], w[1]) and _close(g[2], w[2]), (where, g, w)
        if ref is None:
            assert g[3] == 0.0 and w[3] == 0.0, (where, g, w)
        else:
            _, n, S = ref.score(" ".join(t2c[t] for t in g[0]), bos=True, eos=eos)
            assert abs(g[3] - w[3]) <= 2.0 ** -52 * n * S, (where, g, w)
        assert g[4] == w[4], (where, g, w)


def _lists(raw, B, beam):
    pre, plen, total, ctc, lms, bias, bad = [x.cpu().numpy() for x in raw]
    assert int(bad[0]) == 0
    return [[(tuple(pre[b, i, : plen[b, i]].tolist()), float(total[b, i]), float(ctc[b, i]), float(lms[b, i]), float(bias[b, i]))
             for i in range(beam) if plen[b, i] >= 0] for b in range(B)]


def _check_missing(raw, n_real, with_lm):
    """Slots behind the n_real[b] prefixes that exist: length -1, scores and bias -inf - and no others."""
    _, plen, total, ctc, lms, bias, _ = [x.cpu().numpy() for x in raw]
    for b, n in enumerate(n_real):
        assert (plen[b, :n] >= 0).all() and (plen[b, n:] == -1).all(), (b, plen[b])
        for x in (total, ctc, bias) + ((lms,) if with_lm else ()):
            assert np.isfinite(x[b, :n]).all() and (x[b, n:] == NEG).all(), (b, x[b])


@pytest.mark.parametrize("B,T,V,beam,sharp,order", R.CASES)
def test_biased_beam_equals_the_yardstick(tmp_path, B, T, V, beam, sharp, order):
    from openeat_amd import hip, ops
    logits, lens, path, t2c = R.make_case(tmp_path, B, T, V, beam, sharp, order)
    ref = ngram_ref.RefLM(path)
    lm = NgramLM(path, t2c)
    ref_graph = BR.case_graph(logits, lens, V, beam)
    graph = _device_graph(ref_graph)
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    dlens = lens.to(DEV)
    plm = R.PrefixLM(ref, t2c)
    fired = 0
    for use_lm in (True, False):
        for lw, lb in BR.WEIGHTS:
            for final in (True, False):
                where = (use_lm, lw, lb, final)
                raw = hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, lm if use_lm else None, lw, lb, True, final, raw=True)
                torch.cuda.synchronize()
                got = _lists(raw, B, beam)
                gaps = []
                for b in range(B):
                    want, gap = BR.search(hp[b, : lens[b]], hi[b, : lens[b]], beam, ref_graph, plm if use_lm else None, lw, lb, True, final)
                    gaps.append(gap)
                    assert gap >= GAP_FLOOR, (where, b, gap)                # the case is decidable on this top-k too
                    _compare(got[b], want, ref if use_lm else None, t2c, True, where + (b,))
                    fired += sum(h[4] != 0.0 for h in want)
                _check_missing(raw, [len(u) for u in got], use_lm)
                print(f"lm {use_lm} weights ({lw}, {lb}) final {final}: smallest non-zero gap {min(gaps):.3g}")
    assert fired > 0
    # the list form returns the same
    assert hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, None, lw, lb, True, final) == got
    if (B, T, V) == R.CASES[0][:3]:                                         # the zero-frame utterance: the one empty prefix
        assert [(h[0], h[4]) for h in got[1]] == [((), 0.0)]
    # no lengths given: every utterance uses all T frames
    got_all = hip.ctc_prefix_beam_ctx_device(top_p, top_i, None, beam, graph, lm, 0.5, 0.0, True, False)
    for b in range(B):
        want, _ = BR.search(hp[b], hi[b], beam, ref_graph, plm, 0.5, 0.0, True, False)
        assert [(h[0], h[4]) for h in got_all[b]] == [(h[0], h[4]) for h in want], b


def _bits(x):
    return x.contiguous().view(torch.int64)


def _used(pre, plen):
    return pre[torch.arange(pre.shape[2], device=pre.device).view(1, 1, -1) < plen.unsqueeze(2)]


@pytest.mark.parametrize("B,T,V,beam,sharp,order", R.CASES)
def test_empty_and_all_zero_graphs_are_the_searches_without_a_graph(tmp_path, B, T, V, beam, sharp, order):
    """Bit for bit: with the LM arguments the LM-fused search's lists, order, total, ctc and lm; without an LM and without a
    length bonus the plain search's lists and scores."""
    from openeat_amd import hip, ops
    logits, lens, path, t2c = R.make_case(tmp_path, B, T, V, beam, sharp, order)
    lm = NgramLM(path, t2c)
    rng = np.random.default_rng(3)
    phrases = sorted({tuple(int(t) for t in rng.integers(1, V, int(rng.integers(1, 5)))) for _ in range(10)})
    graphs = [ContextGraph([], 0.37), ContextGraph(phrases, 0.0, [0.0] * len(phrases))]
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    dlens = lens.to(DEV)
    plain = hip.ctc_prefix_beam_device(top_p, top_i, dlens, beam, raw=True)
    for graph in graphs:
        for final in (True, False):
            for lw, lb in R.WEIGHTS:
                for eos in (True, False):
                    want = hip.ctc_prefix_beam_lm_device(top_p, top_i, dlens, beam, lm, lw, lb, eos, raw=True)
                    got = hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, lm, lw, lb, eos, final, raw=True)
                    where = (graph.n_states, final, lw, lb, eos)
                    assert int(got[6][0]) == 0 and int(want[5][0]) == 0
                    assert torch.equal(got[1], want[1]) and torch.equal(_used(got[0], got[1]), _used(want[0], want[1])), where
                    for g, w in zip(got[2:5], want[2:5]):
                        assert torch.equal(_bits(g), _bits(w)), where
                    assert torch.equal(got[5], torch.where(got[1] >= 0, 0.0, NEG).double()), where
            got = hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, None, 0.7, 0.0, True, final, raw=True)
            assert int(got[6][0]) == 0 and int(plain[3][0]) == 0
            assert torch.equal(got[1], plain[1]) and torch.equal(_used(got[0], got[1]), _used(plain[0], plain[1]))
            assert torch.equal(_bits(got[3]), _bits(plain[2])) and torch.equal(_bits(got[2]), _bits(plain[2]))


def test_exact_ties_under_biasing_keep_insertion_order(tmp_path):
    """Uniform frames and single-token phrases that all score 0.5: whole groups of prefixes share a total exactly; the device
    resolves every tie as the dict loop's stable sort does, with the tie LM and without one."""
    from openeat_amd import hip, ops
    logits, lens, path, t2c, beam = R.tie_case(tmp_path)
    V = logits.shape[2]
    ref = ngram_ref.RefLM(path)
    lm = NgramLM(path, t2c)
    ref_graph = BR.make_graph([(t,) for t in range(1, V)], 0.5)
    graph = _device_graph(ref_graph)
    assert all(float(s) == 0.5 for s in ref_graph[1])
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    plm = R.PrefixLM(ref, t2c)
    tied = 0
    for use_lm in (True, False):
        for lw, lb in ((0.5, 0.0), (0.5, 1.0)):
            got = hip.ctc_prefix_beam_ctx_device(top_p, top_i, lens.to(DEV), beam, graph, lm if use_lm else None, lw, lb, True, True)
            for b in range(logits.shape[0]):
                want, gap = BR.search(hp[b, : lens[b]], hi[b, : lens[b]], beam, ref_graph, plm if use_lm else None, lw, lb, True, True)
                assert gap >= GAP_FLOOR
                tied += sum(x[1] == y[1] for x, y in zip(want, want[1:]))
                _compare(got[b], want, ref if use_lm else None, t2c, True, (use_lm, lw, lb, b))
    assert tied > 0                                                         # there were exact ties to resolve


def test_a_lone_zero_frame_utterance():
    from openeat_amd import hip
    beam, T = 4, 5
    top_p = torch.zeros(1, T, beam, device=DEV)
    top_i = torch.arange(beam, device=DEV).repeat(1, T, 1)
    graph = ContextGraph([(1, 2), (3,)], 0.37)
    for final in (True, False):
        raw = hip.ctc_prefix_beam_ctx_device(top_p, top_i, torch.zeros(1, dtype=torch.int32, device=DEV), beam, graph, final=final, raw=True)
        torch.cuda.synchronize()
        assert _lists(raw, 1, beam) == [[((), 0.0, 0.0, 0.0, 0.0)]]
        _check_missing(raw, [1], False)


def test_one_capture_replayed_twice_gives_the_eager_bits(tmp_path):
    from openeat_amd import hip, ops
    B, T, V, beam, sharp, order = R.CASES[0]
    logits, lens, path, t2c = R.make_case(tmp_path, B, T, V, beam, sharp, order)
    lm = NgramLM(path, t2c)
    graph = _device_graph(BR.case_graph(logits, lens, V, beam))
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    dlens = lens.to(DEV)
    for use in (lm, None):
        eager = [x.clone() for x in hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, use, 0.3, 0.8, True, False, raw=True)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, use, 0.3, 0.8, True, False, raw=True)
        for _ in range(2):
            for x in out[:6]:
                x.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            plen = eager[1]
            assert torch.equal(out[1], plen) and int(out[6][0]) == 0
            for e, o in zip(eager[2:6], out[2:6]):
                assert torch.equal(_bits(e), _bits(o))
            assert torch.equal(_used(eager[0], plen), _used(out[0], plen))


def test_bad_arguments_are_reported_not_launched(tmp_path):
    from openeat_amd import hip
    path = str(tmp_path / "s.arpa")
    words = ngram_ref.random_arpa(path, 2, 10, 30, np.random.default_rng(1))
    lm = NgramLM(path, ["<blank>"] + words)
    graph = ContextGraph([(1, 2), (2, 3, 4)], 0.37)
    B, T = 2, 6
    top_p = torch.zeros(B, T, 17, device=DEV)
    top_i = torch.zeros(B, T, 17, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="beam must be 1..16"):
        hip.ctc_prefix_beam_ctx_device(top_p, top_i, None, 17, graph)
    ws = torch.zeros(B * T * 4 * 2 + 1, dtype=torch.int32, device=DEV)
    pre = torch.zeros(B, 4, T, dtype=torch.int32, device=DEV)
    plen = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    sc = [torch.zeros(B, 4, dtype=torch.float64, device=DEV) for _ in range(4)]
    capacity = hip.context_graph(graph, DEV).capacity

    def call(model=(), ctx=(), lw=0.5, lb=0.0, bias_=sc[3]):
        """model / ctx: the fields of the oe_ngram_model / the oe_context_graph that are spoiled; None: the search without one."""
        def spoiled(struct, fields):
            for k, v in dict(fields).items():
                setattr(struct, k, v)
            return struct

        hip.prefix_beam(hip.prefix_beam_args(top_p, top_i, None, 4, T, ws, pre, plen, sc[0], sc[1], sc[2], bias_,
                                             lm=None if model is None else spoiled(hip.ngram_model(lm, DEV), model),
                                             ctx=None if ctx is None else spoiled(hip.context_graph(graph, DEV), ctx),
                                             lm_weight=lw, length_bonus=lb, eos=True, final=True))

    for kw, message in ((dict(model=dict(order=6)), "order must be 1..5"), (dict(model=dict(table=None)), "null pointer"),
                        (dict(ctx=dict(edges=None)), "null pointer"), (dict(bias_=None), "null pointer"), (dict(lw=float("nan")), "finite"),
                        (dict(lb=float("inf")), "finite"), (dict(model=None, lb=float("inf")), "finite"),
                        (dict(ctx=dict(c=float("nan"))), "finite"), (dict(ctx=dict(c=-1.0)), ">= 0"), (dict(ctx=dict(n_states=0)), "n_states"),
                        (dict(ctx=dict(n_states=(1 << 20) + 1)), "n_states"), (dict(ctx=dict(capacity=capacity + 1)), "power of two"),
                        (dict(ctx=dict(capacity=0)), "power of two"), (dict(ctx=dict(max_probe=-1)), "max_probe"),
                        (dict(ctx=dict(max_probe=capacity)), "max_probe"),
                        # the plain search has no weights to ignore; a model / a graph alone, with a table missing
                        (dict(model=None, ctx=None, lw=0.5, lb=0.0), "plain search"), (dict(model=None, ctx=None, lw=0.0, lb=0.5), "plain search"),
                        (dict(ctx=None, model=dict(table=None)), "null pointer"), (dict(model=None, ctx=dict(fail=None)), "null pointer")):
        with pytest.raises(RuntimeError, match=message):
            call(**kw)
    torch.cuda.synchronize()
    assert int(plen.abs().sum()) == 0 and all(float(x.abs().sum()) == 0.0 for x in sc)      # nothing ran


# ------------------------------------------------------------------ through the model ---------------------------------
def _model_graph(V):
    rng = np.random.default_rng(8)
    phrases = [(9, 35, 9)] + sorted({tuple(int(t) for t in rng.integers(1, V, int(rng.integers(2, 5)))) for _ in range(5)})
    scores = rng.uniform(0.5, 3.0, len(phrases)).astype(np.float32)
    return BR.make_graph(phrases, 0.37, scores)


def test_model_ctc_context_beam_search_equals_the_yardstick(tmp_path):
    from openeat_amd import ops
    model, V = _model()
    lm, ref, t2c = _built_lm(tmp_path, V, 51)
    ref_graph = _model_graph(V)
    graph = _device_graph(ref_graph)
    feats, flen = _ragged(37, [97, 83, 64, 41, 23])
    beam, lw, lb = 4, 0.5, 0.2
    with torch.no_grad():
        encoder_out, encoder_mask, _ = model._encode(feats, flen)
        lens = encoder_mask.squeeze(1).sum(1).cpu().tolist()
        top_p, top_i = ops.topk_rows(model.ctc.logits(encoder_out), beam, log_softmax=True)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    plm = R.PrefixLM(ref, t2c)
    fired = 0
    for use_lm in (True, False):
        got = model.ctc_context_beam_search(feats, flen, beam, graph, lm if use_lm else None, lw, lb)
        for b in range(len(lens)):
            want, gap = BR.search(hp[b, : lens[b]], hi[b, : lens[b]], beam, ref_graph, plm if use_lm else None, lw, lb, True, True)
            print(f"lm {use_lm} utterance {b}: {lens[b]} frames, smallest non-zero gap {gap:.3g}")
            _compare(got[b], want, ref if use_lm else None, t2c, True, (use_lm, b))
            fired += sum(h[4] != 0.0 for h in want)
    assert fired > 0
    with pytest.raises(ValueError):
        model.ctc_context_beam_search(feats, flen, 17, graph)
    with pytest.raises(ValueError):
        model.ctc_context_beam_search(feats, flen, beam, None)
    with pytest.raises(ValueError):
        model.ctc_context_beam_search(feats, flen, beam, graph, lm=torch.nn.Identity())


def test_rescoring_with_a_context_graph(tmp_path, monkeypatch):
    """attention_rescoring_batch(context=graph): eager, first sight under graphs and replay return the same tokens, each of
    them a member of the biased n-best; context=None is the call without the parameter, graph-cache keys included."""
    from openeat_amd.models import asr_model
    model, V = _model()
    lm, _, _ = _built_lm(tmp_path, V, 51)
    graph = _device_graph(_model_graph(V))
    feats, flen = _ragged(41, [97, 83, 64, 41, 23])
    beam = 4
    kw = dict(ctc_weight=0.5, reverse_weight=0.3, lm=lm, lm_weight=3.0)
    fp = dict(first_pass_lm=True, first_pass_lm_weight=0.7, length_bonus=0.4)
    with torch.no_grad():
        parent = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, **kw)
        parent_g = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, **kw)
        keys_before = set(model._decode_graphs)
        none = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, context=None, **kw)
        none_g = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, context=None, **kw)
        assert set(model._decode_graphs) == keys_before                     # and the search in the key has neither LM nor graph
        assert all(len(k) == 3 and k[2] == PrefixSearch(beam) for k in keys_before if k[0] == "s1")
        eager = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, context=graph, **kw)
        first = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, context=graph, **kw)
        replay = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, context=graph, **kw)
        nbest = model.ctc_context_beam_search(feats, flen, beam, graph)
        eager_lm = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, context=graph, **kw, **fp)
        first_lm = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, context=graph, **kw, **fp)
        replay_lm = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, context=graph, **kw, **fp)
        nbest_lm = model.ctc_context_beam_search(feats, flen, beam, graph, lm, 0.7, 0.4)
    assert none == parent and none_g == parent and parent_g == parent
    assert first == eager and replay == eager and first_lm == eager_lm and replay_lm == eager_lm
    for b in range(len(eager)):
        assert tuple(eager[b]) in {h[0] for h in nbest[b]}, (b, eager[b])
        assert tuple(eager_lm[b]) in {h[0] for h in nbest_lm[b]}, (b, eager_lm[b])
    specs = [k[2] for k in model._decode_graphs if k[0] == "s1"]
    assert any(s.lm is None and (s.lm_weight, s.length_bonus, s.eos) == (0.0, 0.0, True) and s.context is graph for s in specs)
    assert any(s.lm is lm and (s.lm_weight, s.length_bonus, s.eos) == (0.7, 0.4, True) and s.context is graph for s in specs)
    with pytest.raises(ValueError):
        model.attention_rescoring_batch(feats, flen, 17, context=graph, **kw)
    monkeypatch.setattr(asr_model, "DEVICE_BEAM", False)
    with pytest.raises(ValueError):
        model.attention_rescoring_batch(feats, flen, beam, context=graph, **kw)
    alive = weakref.ref(lm)                                                 # the keys hold the LM and the graph themselves: the
    del lm, kw, specs                                                       # tables a cached capture points at outlive the caller's
    gc.collect()
    assert any(k[0] == "s1" and k[2].lm is alive() is not None for k in model._decode_graphs)


def test_stage_two_adds_the_final_bias(tmp_path):
    """What attention_rescoring_batch(context=graph) hands to the score mix is the n-best lists' final bias, -inf for a missing
    slot, and the mix ADDS it: a bias that favours one slot by more than any score differs makes that slot the pick."""
    model, V = _model()
    graph = _device_graph(_model_graph(V))
    feats, flen = _ragged(41, [97, 83, 64, 41, 23])
    B, beam = 5, 4
    kw = dict(ctc_weight=0.5, reverse_weight=0.3)
    seen = []
    mix = model._rescore_scores
    model._rescore_scores = lambda *a: seen.append(a[-1].clone()) or mix(*a)
    with torch.no_grad():
        model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, context=graph, **kw)
        model._rescore_scores = mix
        nbest = model.ctc_context_beam_search(feats, flen, beam, graph)
        want = torch.tensor([[nb[i][4] if i < len(nb) else NEG for i in range(beam)] for nb in nbest], dtype=torch.float64)
        assert len(seen) == 1 and torch.equal(seen[0].cpu().view(B, beam), want) and float(want[want > NEG].abs().sum()) > 0.0
        encoder_out, encoder_mask, pre, plen, ctc, bad, bias = model._rescore_stage1(feats, flen, PrefixSearch(beam, None, graph))
        Lm = max(int(plen.max()), 1)
        assert int(bad[0]) == 0
        for slot in range(beam):
            favour = torch.full((B, beam), -1.0e6, dtype=torch.float64, device=DEV)
            favour[:, slot] = 0.0
            toks, n, _ = model._rescore_stage2(encoder_out, encoder_mask, pre, plen, ctc, Lm, beam, 0.5, 0.3, None, 0.0, favour.view(-1))
            toks, n = toks.cpu(), n.cpu().tolist()
            for b in range(B):
                if slot < len(nbest[b]):
                    assert tuple(toks[b, : n[b]].tolist()) == nbest[b][slot][0], (slot, b)


def test_stage_one_is_the_public_search_on_the_same_top_k(tmp_path):
    """_rescore_stage1(spec) for the plain, the LM-fused, the biased and the LM-fused biased search: prefixes (within their
    lengths), lengths, CTC scores and bias are what the matching public hip.ctc_prefix_beam_*_device(raw=True) returns on the
    same top-k, bit for bit; no bias without a graph; the status word is 0."""
    from openeat_amd import hip, ops
    model, V = _model()
    lm, _, _ = _built_lm(tmp_path, V, 51)
    graph = _device_graph(_model_graph(V))
    feats, flen = _ragged(41, [97, 83, 64, 41, 23])
    B, beam, lw, lb = 5, 4, 0.7, 0.4
    with torch.no_grad():
        encoder_out, encoder_mask, _ = model._encode(feats, flen)
        lens = encoder_mask.squeeze(1).sum(1).to(torch.int32)
        top_p, top_i = ops.topk_rows(model.ctc.logits(encoder_out), beam, log_softmax=True)
        plain = hip.ctc_prefix_beam_device(top_p, top_i, lens, beam, raw=True)
        fused = hip.ctc_prefix_beam_lm_device(top_p, top_i, lens, beam, lm, lw, lb, raw=True)
        biased = hip.ctc_prefix_beam_ctx_device(top_p, top_i, lens, beam, graph, None, 0.0, lb, raw=True)
        both = hip.ctc_prefix_beam_ctx_device(top_p, top_i, lens, beam, graph, lm, lw, lb, raw=True)
        # (spec; the public search's prefixes, lengths, CTC scores, bias, status word)
        cases = [(PrefixSearch(beam), plain[0], plain[1], plain[2], None, plain[3]),
                 (PrefixSearch(beam, lm, None, lw, lb), fused[0], fused[1], fused[3], None, fused[5]),
                 (PrefixSearch(beam, None, graph, 0.0, lb), biased[0], biased[1], biased[3], biased[5], biased[6]),
                 (PrefixSearch(beam, lm, graph, lw, lb), both[0], both[1], both[3], both[5], both[6])]
        fired = 0
        for spec, w_pre, w_plen, w_ctc, w_bias, w_bad in cases:
            where = spec.plan
            enc, mask, pre, plen, ctc, bad, bias = model._rescore_stage1(feats, flen, spec)
            assert int(bad[0]) == 0 and int(w_bad[0]) == 0, where
            assert pre.shape == (B * beam, w_pre.shape[2]) and plen.shape == ctc.shape == (B * beam,), where
            assert torch.equal(plen.view(B, beam), w_plen) and int((w_plen >= 0).sum()) > 0, where
            assert torch.equal(_used(pre.view(B, beam, -1), w_plen), _used(w_pre, w_plen)), where
            assert torch.equal(ctc.view(B, beam), w_ctc) and torch.equal(_bits(ctc.view(B, beam)), _bits(w_ctc)), where
            if w_bias is None:
                assert bias is None, where
            else:
                assert bias.shape == (B * beam,) and torch.equal(_bits(bias.view(B, beam)), _bits(w_bias)), where
                fired += int((w_bias[w_plen >= 0] != 0).sum())
        assert fired > 0                                                    # the graph's phrases really scored
