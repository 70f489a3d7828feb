"""CPU: the float64 restatement of oe_ctc_graph_beam_logp (ctc_graph_beam_logp_ref.py) against itself - the fast formulation
against the naive one, both against the enumerator and against ctc_graph_logp_ref.graph_logp without a beam, the occupancy
rows, a central finite difference on guard-banded inputs - and the host tables oe_beam_logp_graph reads against
_group_tables.  The inputs the GPU test relies on are checked here to satisfy the conditions it asserts."""
import numpy as np
import pytest

import ctc_graph_beam_logp_ref as P
import ctc_graph_logp_ref as R
from openeat_amd.utils import decoding_graph as DG
from openeat_amd.utils.decoding_graph import DecodingGraph, GraphSet

INF = float("inf")


def recipe(seed, Q, A, V, T):
    rng = np.random.default_rng(seed)
    g = R.random_graph(rng, Q, A, V)
    return g, rng.normal(size=(T, V)) * 2.0


def lexicon(n_words, V, seed, large=False):
    rng = np.random.default_rng(seed)
    words = set()
    while len(words) < n_words:
        words.add(tuple(int(x) for x in rng.integers(1, V, size=int(rng.integers(1, 5)))))
    words = sorted(words)
    return DecodingGraph.from_phrases(words, weights=[-0.05 * (i % 9) for i in range(len(words))], loop=True, large=large)


@pytest.mark.parametrize("beam", [3.0, 8.0, INF])
def test_fast_formulation_equals_the_naive_one(beam):
    for seed, (Q, A, V, T) in enumerate(((12, 40, 9, 12), (40, 200, 20, 16), (5, 30, 4, 9))):
        g, logits = recipe(seed, Q, A, V, T)
        lp = R.log_softmax(logits)
        a, b = P.pruned_logp(lp, g, beam), P.pruned_logp_fast(lp, g, beam)
        assert a["survivors"] == b["survivors"] and a["cut"] == b["cut"]
        assert abs(a["logz"] - b["logz"]) <= 1e-10 and np.abs(a["occ"] - b["occ"]).max() <= 1e-11
        assert abs(a["gap"] - b["gap"]) <= 1e-9 or (a["gap"] == b["gap"] == np.inf)
    g = lexicon(60, 7, 3)                                                    # a hub: node 0 has 60 incoming arcs of 6 labels
    lp = R.log_softmax(np.random.default_rng(5).normal(size=(14, 7)) * 2.0)
    a, b = P.pruned_logp(lp, g, beam), P.pruned_logp_fast(lp, g, beam)
    assert a["survivors"] == b["survivors"] and abs(a["logz"] - b["logz"]) <= 1e-10 and np.abs(a["occ"] - b["occ"]).max() <= 1e-11


def test_against_the_enumerator_and_the_unpruned_restatement():
    rng = np.random.default_rng(11)
    for _ in range(4):
        g = R.random_graph(rng, int(rng.integers(2, 5)), int(rng.integers(3, 9)), 4, final_p=0.6)
        lp = R.log_softmax(rng.normal(size=(5, 4)) * 1.5)
        want = R.enumerate_logz(lp, g)
        for fn in (P.pruned_logp, P.pruned_logp_fast):
            got = fn(lp, g, INF)
            assert (got["logz"] == want == -np.inf) or abs(got["logz"] - want) <= 1e-10
            assert got["cut"] == 0 and got["gap"] == np.inf
    g, logits = recipe(2, 40, 200, 20, 16)
    lp = R.log_softmax(logits)
    full = R.graph_logp(lp, g)
    for fn in (P.pruned_logp, P.pruned_logp_fast):
        got = fn(lp, g, INF)
        assert abs(got["logz"] - full["logz"]) <= 1e-10 and np.abs(got["occ"] - full["occ"]).max() <= 1e-11
    assert P.pruned_logp(lp[:0], g, 4.0)["logz"] == -np.inf                  # no frames: infeasible


def test_occupancy_rows_sum_to_one_and_pruning_only_removes_mass():
    for seed in range(3):
        g, logits = recipe(seed, 40, 200, 20, 16)
        lp = R.log_softmax(logits)
        full = R.graph_logp(lp, g)["logz"]
        for beam in (4.0, 12.0):
            res = P.pruned_logp(lp, g, beam)
            if np.isfinite(res["logz"]):
                assert np.abs(res["occ"].sum(1) - 1.0).max() <= 1e-12
            assert res["logz"] <= full + 1e-12 and res["cut"] > 0


@pytest.mark.parametrize("seed", [1, 6, 7, 8])
def test_finite_difference_on_guard_banded_inputs(seed):
    """(12, 40, 9, 12) at beam 4: the gap keeps every state 0.02 away from its threshold, so a step of 1e-5 moves no state
    across one, and logz is differentiable with the gradient occ - softmax."""
    Q, A, V, T, beam = 12, 40, 9, 12, 4.0
    g, logits = recipe(seed, Q, A, V, T)
    res = P.pruned_logp(R.log_softmax(logits), g, beam)
    print(f"seed {seed}: gap {res['gap']:.4f} cut {res['cut']} survivors {res['survivors']}")
    assert res["gap"] >= 0.02 and 100 <= res["cut"] <= 250 and np.isfinite(res["logz"])
    want = res["occ"] - np.exp(R.log_softmax(logits))
    rng = np.random.default_rng(seed)
    eps = 1e-5
    for _ in range(25):
        t, v = int(rng.integers(0, T)), int(rng.integers(0, V))
        hi, lo = logits.copy(), logits.copy()
        hi[t, v] += eps
        lo[t, v] -= eps
        fd = (P.pruned_logp(R.log_softmax(hi), g, beam)["logz"] - P.pruned_logp(R.log_softmax(lo), g, beam)["logz"]) / (2 * eps)
        assert abs(fd - want[t, v]) <= 1e-6, (t, v, fd, want[t, v])


def test_the_inputs_of_the_gpu_test_meet_its_conditions():
    """What was measured for the random shapes when the GPU cases were chosen: sensitivity to the beam (the restatement at beam +- 1e-3) and the
    effect of pruning."""
    for seed in (1, 2, 3):
        g, logits = recipe(seed, 40, 200, 20, 16)
        lp = R.log_softmax(logits)
        mid, lo, hi = (P.pruned_logp(lp, g, 12.0 + d) for d in (0.0, -1e-3, 1e-3))
        assert mid["logz"] == lo["logz"] == hi["logz"] and np.array_equal(mid["occ"], lo["occ"]) and np.array_equal(mid["occ"], hi["occ"])
        assert 200 <= mid["cut"] <= 500
        assert 5e-5 <= np.abs(mid["occ"] - R.graph_logp(lp, g)["occ"]).max() <= 1e-3


def test_group_tables_of_a_graph_equal_those_of_its_set():
    rng = np.random.default_rng(3)
    for gr in (R.random_graph(rng, 9, 40, 6), lexicon(40, 6, 1), DecodingGraph.token_loop(12), DecodingGraph.linear([3, 3, 1])):
        in_grp, in_xg, out_grp, out_xg, inv = gr.host_group_tables()
        t = GraphSet([gr]).graph_tables(0)
        A, U = gr.num_arcs, len(gr.cols)
        assert np.array_equal(in_xg, t["in_xg"]) and np.array_equal(out_xg, t["out_xg"])
        assert np.array_equal(inv, GraphSet([gr]).tables["inv"])
        for grp, perm, gstart, node in ((in_grp, t["in_perm"], t["in_gstart"], gr.dst), (out_grp, t["out_perm"], t["out_gstart"], gr.src)):
            assert grp.dtype == np.int32 and grp.shape == (A,)
            for a in range(A):
                lo, hi = int(gstart[grp[a]]), int(gstart[grp[a] + 1])
                assert a in perm[lo:hi].tolist()
            key = node.astype(np.int64) * (U + 1) + gr.col                   # one group per (node, col), numbered in key order
            assert np.array_equal(grp, np.searchsorted(np.unique(key), key))
        again = gr.host_group_tables()
        again[0][:] = -7                                                     # a copy: the cache is not the caller's to change
        assert np.array_equal(gr.host_group_tables()[0], in_grp)
    big = lexicon(300, 30, 2, large=True)
    assert big.large and len(big.host_group_tables()[0]) == big.num_arcs


def test_graph_set_limits_are_unchanged():
    assert (DG.LOGP_MAX_NODES, DG.LOGP_MAX_ARCS) == (4096, 5120) and (GraphSet.MAX_NODES, GraphSet.MAX_ARCS) == (4096, 5120)
    with pytest.raises(ValueError):
        GraphSet([DecodingGraph(DG.LOGP_MAX_NODES + 1, [(0, 1, 1, 0.0)], {1: 0.0})])
    with pytest.raises(ValueError):
        GraphSet([DecodingGraph(2, [(0, 1, 1 + i % 7, 0.0) for i in range(DG.LOGP_MAX_ARCS + 1)], {1: 0.0})])
