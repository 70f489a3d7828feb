"""CPU: the yardstick of the joint CTC/attention search with hotword biasing (joint_ctx_search_ref.py) - its running hits and
bias against the brute-force definition and against the automaton of ContextGraph, the search with an empty graph against the
yardsticks without one, the gaps of every search the GPU test compares (test_joint_ctx_search_gpu.py asserts them again, here
they are examined without a device), and the host-side surface of oe_context_next, ops.context_next and joint_beam_search.
No compute is launched here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ctc_bias_beam_ref as B
import ctc_prefix_score_ref as ref
import joint_ctx_search_ref as X
import joint_lm_search_ref as R
from conftest import ROOT

EOS = 9


def test_running_hits_and_bias_are_the_definition():
    """Walking random prefixes candidate by candidate: (hits', bias') of every step is bias_direct of the extended prefix
    (final / not final), the <eos> candidate is the un-extended prefix with the credit dropped - and ContextGraph's automaton
    (state, hits, pend) gives the same bits."""
    from openeat_amd.utils.context_graph import ContextGraph
    rng = np.random.default_rng(3)
    phrases = [(1, 2, 3), (2, 3), (3,), (2, 3, 4), (5, 5), (5, 5, 5, 1), (7, 1, 2)]
    scores = rng.uniform(0.2, 2.5, len(phrases)).astype(np.float32)
    graph = B.make_graph(phrases, B.C, scores)
    cg = ContextGraph(phrases, B.C, scores)
    for _ in range(40):
        prefix = tuple(int(t) for t in rng.integers(0, 9, int(rng.integers(0, 12))))
        g, s, hits = (), 0, 0.0
        for tok in prefix:
            h, b = X.ctx_next(graph, g, tok, EOS)
            assert h == B.bias_direct(graph, g + (tok,), True) and b == B.bias_direct(graph, g + (tok,), False)
            s = cg.step(s, tok)
            t = s
            while t:
                hits += float(cg.score[t])
                t = int(cg.link[t])
            assert hits == h and hits + float(cg.context_score) * int(cg.pend[s]) == b
            g = g + (tok,)
            assert cg.bias(g, True) == h and cg.bias(g, False) == b
            he, be = X.ctx_next(graph, g, EOS, EOS)
            assert he == be == B.bias_direct(graph, g, True)


@pytest.mark.parametrize("context_prebeam", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_an_empty_graph_is_the_search_without_one(tmp_path, lam, context_prebeam):
    """No phrases: the n-best of ctc_prefix_score_ref.joint_search and of joint_lm_search, every number exactly; bias is 0."""
    V, eos, T = 6, 5, 7
    plm = R.prefix_lm(*R.make_lm(tmp_path, V, 3, 1))
    empty = B.make_graph([], 0.0)
    found = 0
    for seed in range(3):
        for beam, C, beta in ((1, 2, 0.0), (3, 4, 0.25), (4, V, 0.5)):
            rng = np.random.RandomState(seed)
            x = rng.randn(T, V) * 1.5
            y = x - np.log(np.exp(x).sum(1, keepdims=True))
            x = rng.randn(T + 1, V + 1, V) * 2.0
            tab = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
            att = lambda g: tab[min(len(g), T), (g[-1] + 1) if g else 0]                       # noqa: E731
            want, _ = ref.joint_search(y, T, att, eos, beam, C, lam, beta, T)
            got, _, _ = X.joint_ctx_search(y, T, att, eos, beam, C, lam, beta, T, empty, None, 0.0, True, context_prebeam)
            assert [h[:5] for h in got] == want and all(h[5] == 0.0 and len(h) == 6 for h in got)
            for pre in (True, False):
                want, _, _ = R.joint_lm_search(y, T, att, eos, beam, C, lam, beta, T, plm, 0.7, pre)
                got, _, _ = X.joint_ctx_search(y, T, att, eos, beam, C, lam, beta, T, empty, plm, 0.7, pre, context_prebeam)
                assert [h[:6] for h in got] == want and all(h[6] == 0.0 and len(h) == 7 for h in got)
            found += len(got)
    assert found > 9


def test_a_hotword_overturns_the_decoders_first_choice():
    """The decoder slightly prefers token 1 at every step; the phrase (2, 2, 2) is worth more than the difference.  With two
    candidates the bias reorders what the decoder proposes; with one candidate only the pre-selection with the bias can
    change anything.  The unfinished best hypothesis keeps its pending credit; a finished one has dropped it."""
    V, eos, T = 4, 3, 0
    y = np.zeros((0, V))
    lp = np.log(np.array([0.02, 0.5, 0.4, 0.08])).astype(np.float32)
    att = lambda g: lp                                                                          # noqa: E731
    graph = B.make_graph([(2, 2, 2)], 0.5)
    none = B.make_graph([], 0.0)
    run = lambda C, gr, pre, steps=2: X.joint_ctx_search(y, T, att, eos, 2, C, 0.0, 0.0, steps, gr, None, 0.0, True, pre)[0][0]   # noqa: E731
    assert run(2, none, True)[0] == [1, 1] and run(2, none, False)[0] == [1, 1]
    assert run(2, graph, True)[0] == [2, 2] and run(2, graph, False)[0] == [2, 2]
    assert run(1, graph, False)[0] == [1, 1]                    # the decoder's single proposal stands
    assert run(1, graph, True)[0] == [2, 2]                     # the bias takes part in the proposal
    best = run(2, graph, True)
    assert best[5] == float(np.float32(0.5)) * 2 and abs(best[1] - (2 * float(lp[2]) + 1.0)) < 1e-12
    full = run(2, graph, True, 3)
    # the phrase fired: its score - and its last two tokens begin it again, two tokens of credit
    assert full[0] == [2, 2, 2] and full[5] == float(np.float32(0.5) * np.float32(3)) + float(np.float32(0.5)) * 2
    # <eos> drops the credit: the only candidate of a hypothesis that holds (2, 2)
    h, b = X.ctx_next(graph, (2, 2), eos, eos)
    assert h == b == 0.0 and X.ctx_next(graph, (2,), 2, eos) == (0.0, 1.0)


def test_the_gpu_cases_keep_their_distance(tmp_path):
    """Every search test_joint_ctx_search_gpu.py compares with the yardstick, on the host: the smallest gap between
    neighbouring totals and between the C-th and (C+1)-th pre-selection key stay above what that test asserts (the seeds in
    joint_ctx_search_ref.py were chosen until they did) - and some hotwords fire in every shape."""
    worst_total, worst_key = math.inf, math.inf
    tables, graphs, lms = {}, {}, {}
    fired = {s: 0 for s in X.SHAPES}
    for shape, lam, beam, w, cpre, mode in X.search_cases():
        C, beta = R.WEIGHTS[w]
        if shape not in tables:
            tables[shape] = X.make_tables(shape)
            graphs[shape] = X.case_graph(shape, *tables[shape])
        y, tab, lens = tables[shape]
        V, Tmax = y.shape[2], y.shape[1]
        plm, pre = None, True
        if mode is not None:
            order, pre = mode
            if (V, order) not in lms:
                lms[V, order] = R.make_lm(tmp_path, V, order, R.LM_SEED)
            plm = R.prefix_lm(*lms[V, order])
        for nb, gap, key_gap in X.yardstick(y, tab, lens, graphs[shape], plm, beam, C, lam, beta, Tmax, w, pre, cpre):
            assert gap >= R.TOTAL_GAP and key_gap >= R.KEY_GAP, (shape, lam, beam, w, cpre, mode, gap, key_gap)
            assert cpre or (plm is not None and pre) or key_gap == math.inf
            worst_total, worst_key = min(worst_total, gap), min(worst_key, key_gap)
            fired[shape] += sum(1 for h in nb if B.hits(graphs[shape], h[0]) > 0)
    assert all(n > 0 for n in fired.values()), fired
    c = R.SURVIVOR
    y, tab, lens = X.make_tables("survivor")
    graph = X.survivor_graph(c["V"])
    plm = R.prefix_lm(*R.make_lm(tmp_path, c["V"], c["order"], R.LM_SEED))
    for cpre in (True, False):
        for max_steps in (1, 2, 3, 4, 5):
            for nb, gap, key_gap in X.yardstick(y, tab, lens, graph, plm, c["beam"], c["C"], c["lam"], 0.0, max_steps, c["lm_weight"], True, cpre):
                assert gap >= R.TOTAL_GAP and key_gap >= R.KEY_GAP, ("survivor", cpre, max_steps, gap, key_gap)
                assert [h[4] for h in nb] == [True, False, False] and nb[0][0] == [] and nb[0][6] == 0.0, nb
                assert all(h[6] > 0 for h in nb[1:])
                worst_total, worst_key = min(worst_total, gap), min(worst_key, key_gap)
    print(f"smallest gaps: totals {worst_total:.3g} (asserted {R.TOTAL_GAP}), pre-selection keys {worst_key:.3g} (asserted {R.KEY_GAP})")


def test_entry_point_is_declared_bound_and_validated():
    from openeat_amd import hip, ops
    lib = hip.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "openeat_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+oe_context_next\s*\(", src)
    assert "oe_context_next" in hip.exported_symbols() and hasattr(lib, "oe_context_next")
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "openeat_amd", "lib", "libopeneat_hip.so")), "oe_context_next")
    assert callable(ops.context_next)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def graph(**spoil):
        kw = dict(edges=p, fail=p, out=p, pend=p, capacity=4, max_probe=1, n_states=3, c=0.5)
        kw.update(spoil)
        return hip.ContextGraph(kw["edges"], kw["fail"], kw["out"], kw["pend"], kw["capacity"], kw["max_probe"], kw["n_states"], kw["c"])

    def call(g=None, state=p, hits=p, R_=1, cand=p, C=2, eos_tok=5, out_state=p, out_hits=p, out_bias=p, no_graph=False):
        return lib.oe_context_next(None if no_graph else (graph() if g is None else g), state, hits, R_, cand, C, eos_tok, out_state,
                                   out_hits, out_bias, None)

    for kwargs, say in [(dict(no_graph=True), b"null"), (dict(state=None), b"null"), (dict(hits=None), b"null"),
                        (dict(out_bias=None), b"null"), (dict(g=graph(edges=None)), b"null"), (dict(g=graph(fail=None)), b"null"),
                        (dict(g=graph(out=None)), b"null"), (dict(g=graph(pend=None)), b"null"),
                        (dict(out_state=None), b"together"), (dict(out_hits=None), b"together"),
                        (dict(R_=-1), b"bad shape"), (dict(C=0), b"C must be >= 1"), (dict(C=-3), b"C must be >= 1"),
                        (dict(cand=None, C=0), b"C must be >= 1"), (dict(eos_tok=-2), b"eos_tok"),
                        (dict(g=graph(n_states=0)), b"n_states"), (dict(g=graph(n_states=(1 << 20) + 1)), b"n_states"),
                        (dict(g=graph(capacity=6)), b"capacity"), (dict(g=graph(capacity=1)), b"capacity"),
                        (dict(g=graph(max_probe=4)), b"max_probe"), (dict(g=graph(max_probe=-1)), b"max_probe"),
                        (dict(g=graph(c=-0.5)), b"partial credit"), (dict(g=graph(c=float("nan"))), b"partial credit"),
                        (dict(g=graph(c=float("inf"))), b"partial credit")]:
        assert call(**kwargs) != 0, kwargs
        assert say in lib.oe_last_error(), (kwargs, lib.oe_last_error())
        assert b"oe_context_next" in lib.oe_last_error()
    # nothing to do is not an error and launches nothing
    assert call(R_=0) == 0 and call(R_=0, cand=None, C=6, eos_tok=-1, out_state=None, out_hits=None) == 0


def test_ops_context_next_refuses_what_needs_no_device():
    import torch
    from openeat_amd import ops
    from openeat_amd.utils.context_graph import ContextGraph
    cg = ContextGraph([(1, 2)])
    state, hits = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64)
    with pytest.raises(TypeError, match="CUDA"):
        ops.context_next(cg, state, hits, V=6)
    with pytest.raises(TypeError, match="CUDA"):
        ops.context_next(cg, state, hits, torch.zeros(2, 4, dtype=torch.int32), eos=5)
    with pytest.raises(TypeError, match="ContextGraph"):
        ops.context_next([(1, 2)], state, hits, V=6)


def test_joint_beam_search_refuses_what_is_no_graph():
    import torch
    from openeat_amd.utils import joint_search as js
    logp = torch.zeros(1, 2, 6)
    for context in ([(1, 2)], "hotwords.txt", object()):
        with pytest.raises(ValueError, match="ContextGraph"):
            js.joint_beam_search(logp, None, lambda t, p: logp[:, 0], 1, 2, 5, context=context)
    assert js.BeamState._fields[-3:] == ("cstate", "hits", "bias") and js.BeamState._field_defaults["bias"] is None
