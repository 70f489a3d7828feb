"""CPU: the restatement of oe_ctc_graph_nbest (ctc_graph_nbest_ref.py) against the brute force - every arc path of at most Tb
arcs, scored by ctc_graph_ref.decode on its linear chain - on random tiny graphs (Q <= 4, A <= 8, T <= 5) whose values lie on
the 1/8 grid, where every float32 sum is exact and equal scores really tie; and the host records made of the kernel's outputs."""
import numpy as np
import pytest

import ctc_graph_nbest_ref as N
import ctc_graph_ref as R
from openeat_amd.utils.decoding_graph import DecodingGraph, GraphHypothesis, graph_hypotheses


def grid(rng, n, lo):
    return rng.integers(8 * lo, 1, size=n).astype(np.float64) / 8


def tiny_case(seed):
    """A random graph with self-loops, parallel arcs and ties; node 0 final in a third of the cases."""
    rng = np.random.default_rng(seed)
    Q, A, T, V = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.integers(1, 6)), int(rng.integers(3, 5))
    arcs = [(int(rng.integers(0, Q)) if rng.random() < 0.6 else 0, int(rng.integers(0, Q)), int(rng.integers(1, V)), float(grid(rng, 1, -2)[0]))
            for _ in range(A)]
    finals = {int(q): float(grid(rng, 1, -2)[0]) for q in rng.integers(0, Q, size=max(Q // 2, 1))}
    if seed % 3 == 0:
        finals[0] = -0.5
    g = DecodingGraph(Q, arcs, finals)
    lp = grid(rng, (T, V), -3)
    return g, lp, T, int(rng.integers(1, 6))


SEEDS = list(range(60))


@pytest.mark.parametrize("distinct", [N.ARCS, N.TOKENS])
def test_restatement_equals_the_brute_force(distinct):
    nonempty = short = 0
    for seed in SEEDS:
        g, lp, T, K = tiny_case(seed)
        Tb = T if seed % 5 else max(T - 1, 0)
        got = N.nbest_graph(lp, Tb, g, K, distinct, np.float32)
        want = N.brute_force(lp, Tb, g.num_nodes, g.src, g.dst, g.label, g.w, g.final, distinct)
        n = got["n_hyp"]
        assert n == min(K, len(want)), seed
        assert got["hyp_score"][:n].tolist() == [float(s) for s, _ in want[:n]], seed
        assert np.isneginf(got["hyp_score"][n:]).all() and (got["hyp_len"][n:] == -1).all()
        keys = [p if distinct == N.ARCS else tuple(int(g.label[a]) for a in p) for p in got["paths"]]
        assert len(set(keys)) == n, seed                                 # distinct histories
        for k, path in enumerate(got["paths"]):                          # each path's own best-alignment score is the reported one
            assert N.path_score(lp, Tb, path, g.src, g.dst, g.label, g.w, g.final) == got["hyp_score"][k], (seed, k)
            assert got["hyp_len"][k] == len(path) and got["hyp_arcs"][k, :len(path)].tolist() == list(path)
            assert got["hyp_tokens"][k, :len(path)].tolist() == g.label[list(path)].tolist()
        nonempty += n > 0
        short += n < K
    assert nonempty >= 30 and short >= 5                                 # K larger than the number of accepted paths: n_hyp < K


def test_one_best_equals_the_graph_decode_in_float32():
    for seed in SEEDS:
        g, lp, T, _ = tiny_case(seed)
        ref = R.decode_graph(lp, T, g, np.float32)
        for distinct in (N.ARCS, N.TOKENS):
            got = N.nbest_graph(lp, T, g, 1, distinct, np.float32)
            assert got["hyp_score"][0].tobytes() == np.float32(ref["score"]).tobytes(), seed
            n = ref["n_trav"]
            assert got["n_hyp"] == int(np.isfinite(ref["score"]))
            if got["n_hyp"]:
                assert got["hyp_len"][0] == n and got["hyp_arcs"][0, :n].tolist() == ref["trav_arc"][:n].tolist(), seed


def test_hash_identity_equals_tuple_identity():
    for seed in SEEDS:
        g, lp, T, K = tiny_case(seed)
        for distinct in (N.ARCS, N.TOKENS):
            seen = {}
            a = N.nbest_graph(lp, T, g, K, distinct, np.float32)
            b = N.nbest_graph(lp, T, g, K, distinct, np.float32, identity="hash", keys_seen=seen)
            assert a["paths"] == b["paths"] and np.array_equal(a["hyp_score"], b["hyp_score"]), seed
    assert N.mix(0, 0) == 0xE220A8397B1DCDAF                              # splitmix64's first output from state 0


def test_the_empty_path_is_a_hypothesis():
    g = DecodingGraph(2, [(0, 1, 1, 0.0)], {0: -0.25, 1: 0.0})
    lp = np.array([[-0.125, -2.0], [-0.25, -2.0]])
    got = N.nbest_graph(lp, 2, g, 3, N.ARCS, np.float32)
    assert got["n_hyp"] == 2 and got["hyp_len"].tolist() == [0, 1, -1]
    assert got["hyp_score"][0] == np.float32(-0.625) and (got["hyp_arcs"][0] == -1).all()
    assert got["paths"] == [(), (0,)]


def test_parallel_arcs_merge_in_tokens_mode_only():
    g = DecodingGraph(2, [(0, 1, 1, 0.0), (0, 1, 1, -0.5), (0, 1, 2, -1.0)], {1: 0.0})
    lp = np.zeros((2, 3)) - 1.0
    arcs = N.nbest_graph(lp, 2, g, 4, N.ARCS, np.float32)
    toks = N.nbest_graph(lp, 2, g, 4, N.TOKENS, np.float32)
    assert arcs["n_hyp"] == 3 and toks["n_hyp"] == 2
    assert toks["paths"] == [(0,), (2,)] and toks["hyp_score"][:2].tolist() == [-2.0, -3.0]


def test_max_len_shorter_than_a_path():
    g = DecodingGraph.linear([1, 2, 1])
    lp = np.zeros((4, 3)) - 0.5
    got = N.nbest_graph(lp, 4, g, 2, N.ARCS, np.float32, max_len=2)
    assert got["n_hyp"] == 1 and got["hyp_len"][0] == 3 and got["hyp_tokens"][0].tolist() == [1, 2]


def test_graph_hypothesis_records():
    g = DecodingGraph.from_phrases([[1, 2], [3]], weights=[0.0, -0.5], outputs=["first", "second"])
    lp = np.zeros((3, 4)) - 1.0
    r = N.nbest_graph(lp, 3, g, 3, N.TOKENS, np.float32, max_len=1)
    out = graph_hypotheses(g, [r["n_hyp"], 0], [r["hyp_score"].tolist()] * 2, [r["hyp_len"].tolist()] * 2, [r["hyp_arcs"].tolist()] * 2,
                           [r["hyp_tokens"].tolist()] * 2)
    assert len(out) == 2 and out[1] == [] and len(out[0]) == r["n_hyp"] == 2
    for k, h in enumerate(out[0]):
        assert isinstance(h, GraphHypothesis) and h.rank == k and h.score == float(r["hyp_score"][k])
        assert h.arcs == r["hyp_arcs"][k, :len(h.arcs)].tolist() and h.tokens == [int(g.label[a]) for a in h.arcs]
        assert h.truncated == (r["hyp_len"][k] > 1)
    by_tokens = {tuple(int(g.label[a]) for a in p): p for p in r["paths"]}
    assert set(by_tokens) == {(1, 2), (3,)}
    single = next(h for h in out[0] if h.tokens == [3])
    assert single.outputs == ["second"] and not single.truncated
