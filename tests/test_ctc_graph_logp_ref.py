"""CPU: the float64 restatement of oe_ctc_graph_logp (ctc_graph_logp_ref.py) against the definition (an enumeration of every
labelling x every accepting path), its gradient against central differences, and the host side of the feature:
DecodingGraph.from_alternatives and the GraphSet packing."""
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_graph_logp_ref as R  # noqa: E402
from openeat_amd.utils.decoding_graph import LOGP_MAX_ARCS, LOGP_MAX_NODES, DecodingGraph, GraphSet  # noqa: E402


random_graph = R.random_graph


def test_restatement_equals_the_enumeration():
    rng = np.random.default_rng(11)
    V, feasible = 3, 0
    for i in range(30):
        g = random_graph(rng, int(rng.integers(1, 5)), int(rng.integers(1, 9)), V)
        T = int(rng.integers(1, 6))
        lp = rng.normal(size=(T, V)) * 2.0                              # need not be normalised
        got, want = R.graph_logp(lp, g)["logz"], R.enumerate_logz(lp, g)
        if np.isfinite(want):
            feasible += 1
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (i, got, want)
        else:
            assert got == -np.inf
    assert feasible >= 15


def test_token_loop_by_enumeration_and_zero():
    g = DecodingGraph.token_loop(6)
    rng = np.random.default_rng(3)
    lp = rng.normal(size=(4, 6))
    assert abs(R.graph_logp(lp, g)["logz"] - R.enumerate_logz(lp, g)) <= 1e-12
    logits = rng.normal(size=(1, 7, 6)) * 3
    logp, grad = R.logp_and_grad(logits, [7], g)
    assert abs(logp[0]) <= 1e-12 and np.abs(grad).max() <= 1e-12
    res = R.graph_logp(R.log_softmax(logits[0]), g)
    assert np.allclose(res["occ"], np.exp(R.log_softmax(logits[0])), atol=1e-12)


def test_gradient_against_central_differences_and_occupancy_rows():
    rng = np.random.default_rng(5)
    V, T, checked = 4, 5, 0
    for i in range(8):
        g = random_graph(rng, 4, 9, V, final_p=0.6)
        logits = rng.normal(size=(1, T, V))
        logp, grad = R.logp_and_grad(logits, [T], g, g=np.array([1.7]))
        if not np.isfinite(logp[0]):
            assert not grad.any()
            continue
        checked += 1
        occ = R.graph_logp(R.log_softmax(logits[0]), g)["occ"]
        assert np.allclose(occ.sum(-1), 1.0, atol=1e-12)
        eps = 1e-6
        for t, v in itertools.product(range(T), range(V)):
            hi, lo = logits.copy(), logits.copy()
            hi[0, t, v] += eps
            lo[0, t, v] -= eps
            num = 1.7 * (R.logp_and_grad(hi, [T], g)[0][0] - R.logp_and_grad(lo, [T], g)[0][0]) / (2 * eps)
            assert abs(num - grad[0, t, v]) <= 1e-7, (i, t, v, num, grad[0, t, v])
    assert checked >= 4


def test_linear_chain_is_the_ctc_loss():
    from oracle.ctc_np import ctc_nll_and_grad
    rng = np.random.default_rng(7)
    B, T, V = 3, 9, 5
    logits = rng.normal(size=(B, T, V))
    targets = np.array([[1, 1, 2, 0], [3, 0, 0, 0], [4, 2, 2, 1]])
    tlens, hlens = [3, 1, 4], [9, 4, 7]
    nll, grad = ctc_nll_and_grad(logits, hlens, targets, tlens)
    graphs = [DecodingGraph.linear(targets[b, :tlens[b]]) for b in range(B)]
    logp, mine = R.logp_and_grad(logits, hlens, graphs, graph_of=[0, 1, 2])
    assert np.allclose(-logp, nll, atol=1e-10) and np.allclose(-mine, grad, atol=1e-10)


def expansions(segments):
    return {tuple(t for alt in choice for t in alt) for choice in itertools.product(*segments)}


@pytest.mark.parametrize("segments", [
    [[[1], []], [[2]], [[1, 2], [3]]],                                      # optional first
    [[[1]], [[2, 3], [3]], [[2], []]],                                      # optional last
    [[[1]], [[2], []], [[3], []], [[1], []], [[2]]],                        # consecutive optional segments
    [[[1], []], [[2], []], [[3]]],
    [[[2]], [[2], [1, 2]], [[2], []], [[1], []]],                           # repeats across the joints; the tail optional
])
def test_from_alternatives_accepts_exactly_the_expansions(segments):
    g = DecodingGraph.from_alternatives(segments)
    want = expansions(segments)
    longest = max(len(x) for x in want)
    for n in range(longest + 2):
        for toks in itertools.product((1, 2, 3), repeat=n):
            frames = [c for t in toks for c in (t, 0)]                      # a blank behind every token: repeats stay apart
            assert g.accepts(frames) == (toks in want), (toks, segments)


def test_from_alternatives_weights_and_errors():
    segments = [[[1], [2, 3]], [[1], []], [[3]]]
    weights = [[-0.25, -1.5], [-0.125, -2.0], [0.5]]
    g = DecodingGraph.from_alternatives(segments, weights)
    for choice in itertools.product(*(range(len(s)) for s in segments)):
        toks = [t for i, j in enumerate(choice) for t in segments[i][j]]
        want = sum(weights[i][j] for i, j in enumerate(choice))
        assert abs(R.path_weight(g, toks) - want) <= 1e-6, (choice, toks)
    with pytest.raises(ValueError):
        DecodingGraph.from_alternatives([[[1], []], [[2], []]])            # the whole transcript can be empty
    with pytest.raises(ValueError):
        DecodingGraph.from_alternatives([[[1], [1]]])
    with pytest.raises(ValueError):
        DecodingGraph.from_alternatives([[list(range(1, LOGP_MAX_NODES + 2))]])
    with pytest.raises(ValueError):
        DecodingGraph.from_alternatives([])


def test_graph_set_round_trips_each_graphs_tables():
    rng = np.random.default_rng(2)
    graphs = [random_graph(rng, 5, 14, 7), DecodingGraph.token_loop(5), DecodingGraph.linear([3, 3, 9]),
              DecodingGraph.from_phrases([[1, 2], [3, 2], [2]], loop=True)]
    s = GraphSet(graphs)
    assert s.num_graphs == 4 and s.Qmax == 5 and s.Amax == 14 and (GraphSet.MAX_NODES, GraphSet.MAX_ARCS) == (LOGP_MAX_NODES, LOGP_MAX_ARCS)
    assert s.cols.tolist() == sorted({int(x) for g in graphs for x in g.label})
    inv = s.tables["inv"]
    assert inv[0] == 0 and all(inv[c] == 1 + k for k, c in enumerate(s.cols)) and (inv >= 0).sum() == len(s.cols) + 1
    U = len(s.cols)
    for i, g in enumerate(graphs):
        t = s.graph_tables(i)
        Q, A = g.num_nodes, g.num_arcs
        for name, want in (("in_ptr", g.in_ptr), ("src", g.src), ("dst", g.dst), ("label", g.label), ("w", g.w), ("final", g.final)):
            assert np.array_equal(t[name], want), (i, name)
        assert np.array_equal(s.cols[t["col"]], g.label)
        for perm, gstart, gptr, xg, node, other in (("in_perm", "in_gstart", "in_gptr", "in_xg", g.dst, g.src),
                                                    ("out_perm", "out_gstart", "out_gptr", "out_xg", g.src, g.dst)):
            assert sorted(t[perm].tolist()) == list(range(A)) and len(t[gstart]) == A + 1 and len(t[gptr]) == Q + 1
            groups = {}
            for q in range(Q):
                for grp in range(t[gptr][q], t[gptr][q + 1]):
                    members = t[perm][t[gstart][grp]:t[gstart][grp + 1]].tolist()
                    assert members and members == sorted(members)
                    assert {int(node[a]) for a in members} == {q} and len({int(g.label[a]) for a in members}) == 1
                    groups[(q, int(g.label[members[0]]))] = (grp, members)
            assert sorted(a for _, m in groups.values() for a in m) == list(range(A))       # every arc in exactly one group
            for a in range(A):
                assert t[xg][a] == groups.get((int(other[a]), int(g.label[a])), (-1, None))[0]
        assert len(t["col_ptr"]) == U + 1 and t["col_ptr"][0] == 0 and t["col_ptr"][U] == A
        for k in range(U):
            members = t["col_perm"][t["col_ptr"][k]:t["col_ptr"][k + 1]].tolist()
            assert members == [a for a in range(A) if g.label[a] == s.cols[k]]
    with pytest.raises(ValueError):
        GraphSet([DecodingGraph.linear(list(range(1, LOGP_MAX_NODES + 1)))])
