"""CPU: the restatement of grammar-constrained CTC decoding (ctc_graph_ref.py) - its float32 run against its float64 run on the
1/8-grid fixtures the GPU tests use (every partial sum is a multiple of 1/8 below 2^17, exact in float32), against the aligner's
restatement on linear chains, against the sum of the row maxima on a token loop, and against a brute force over every frame
labelling - and the graph builders of openeat_amd/utils/decoding_graph.py."""
import numpy as np
import pytest

import ctc_align_ref as AR
import ctc_graph_ref as R
from openeat_amd.utils.decoding_graph import MAX_ARCS, MAX_NODES, DecodingGraph, GraphResult, graph_results

OUTPUTS = ("score", "frames", "arcs", "path_logp", "n_trav", "trav_arc", "trav_start", "trav_end", "trav_logp")


def grid_lp(rng, T, V):
    """Log-probabilities that are multiples of 1/8 in [-8, 0]."""
    return rng.integers(-64, 1, size=(T, V)).astype(np.float64) / 8


def grid_w(rng, n):
    """Weights that are multiples of 1/8 in [-4, 0]."""
    return rng.integers(-32, 1, size=n).astype(np.float64) / 8


def random_graph(rng, Q, A, V, grid=True):
    arcs = [(int(rng.integers(0, Q)), int(rng.integers(0, Q)), int(rng.integers(1, V)), float(w))
            for w in (grid_w(rng, A) if grid else rng.standard_normal(A))]
    finals = {int(q): float(grid_w(rng, 1)[0]) for q in rng.integers(0, Q, size=max(Q // 2, 1))}
    return DecodingGraph(Q, arcs, finals)


def test_float32_equals_float64_on_the_grid():
    rng = np.random.default_rng(3)
    feasible = 0
    for rep in range(12):
        Q, A, V = int(rng.integers(1, 7)), int(rng.integers(1, 15)), int(rng.integers(3, 7))
        T = 5000 if rep == 0 else int(rng.integers(1, 60))
        g = random_graph(rng, Q, A, V)
        lp = grid_lp(rng, T, V)
        a, b = R.decode_graph(lp, T, g, np.float64, max_trav=7), R.decode_graph(lp, T, g, np.float32, max_trav=7)
        for name in OUTPUTS:
            assert np.array_equal(np.asarray(a[name], dtype=np.float64), np.asarray(b[name], dtype=np.float64)), (rep, name)
        assert b["path_logp"].dtype == np.float32
        feasible += a["score"] > -np.inf
    assert feasible >= 6


@pytest.mark.parametrize("y,T", [([1, 2, 3], 9), ([2, 2, 1], 8), ([1, 1, 1], 5), ([], 4), ([1, 2, 3, 4], 3), ([1, 1], 2), ([3], 1),
                                 ([4, 1, 1, 2, 4, 4], 40)])
def test_linear_chain_is_the_aligners_problem(y, T):
    rng = np.random.default_rng(len(y) * 100 + T)
    V = 5
    for lp in (grid_lp(rng, T, V), np.zeros((T, V)), AR.log_softmax(rng.standard_normal((T, V)) * 2)):   # all-zero: every tie there is
        score, states, toks = AR.align(lp, y)
        got = R.decode_graph(lp, T, DecodingGraph.linear(y))
        assert got["score"] == score
        if states is None:
            assert (got["frames"] == -1).all() and got["n_trav"] == 0
        else:
            assert got["frames"].tolist() == toks
            assert got["n_trav"] == len(y) and got["trav_arc"][: len(y)].tolist() == list(range(len(y)))
            start, end = AR.spans(states, len(y))
            assert got["trav_start"][: len(y)].tolist() == start and got["trav_end"][: len(y)].tolist() == end


def test_token_loop_is_best_path_decoding():
    rng = np.random.default_rng(5)
    T, V = 30, 7
    lp = AR.log_softmax(rng.standard_normal((T, V)) * 3)
    got = R.decode_graph(lp, T, DecodingGraph.token_loop(V))
    assert got["score"] == pytest.approx(lp.max(axis=1).sum(), rel=1e-12)
    assert got["frames"].tolist() == lp.argmax(axis=1).tolist()
    lp = grid_lp(rng, T, V)
    assert R.decode_graph(lp, T, DecodingGraph.token_loop(V))["score"] == lp.max(axis=1).sum()


def test_brute_force_over_every_labelling():
    rng = np.random.default_rng(7)
    V, feasible = 3, 0
    for rep in range(40):
        T, Q, A = int(rng.integers(1, 7)), int(rng.integers(1, 5)), int(rng.integers(1, 9))
        g = random_graph(rng, Q, A, V, grid=rep % 2 == 0)
        lp = AR.log_softmax(rng.standard_normal((T, V)) * 2)
        got = R.decode_graph(lp, T, g)
        want = R.brute_force(lp, g.num_nodes, g.src, g.dst, g.label, g.w, g.final)
        assert got["score"] == pytest.approx(want, rel=1e-12, abs=1e-12), rep
        if want > -np.inf:
            feasible += 1
            path = got["frames"].tolist()
            assert g.accepts(path)
            # the restatement's own path reaches its score: lp along it plus the weights of the arcs it enters and the final
            wsum = sum(float(g.w[a]) for a in got["trav_arc"][: got["n_trav"]])
            last = got["arcs"][T - 1]
            end = int(g.dst[last]) if last >= 0 else (int(g.dst[got["trav_arc"][got["n_trav"] - 1]]) if got["n_trav"] else 0)
            assert got["path_logp"].sum() + wsum + float(g.final[end]) == pytest.approx(want, rel=1e-12, abs=1e-12)
        else:
            assert not any(g.accepts(p) for p in ([0] * T, [1] * T, [2] * T))
    assert feasible >= 15


def test_final_weights_and_arc_weights_choose_the_winner():
    lp = np.zeros((2, 3))
    lp[:, 0] = -8.0                                                           # no blank: the arc states decide
    g = DecodingGraph(3, [(0, 1, 1, 0.0), (0, 2, 2, 0.0)], {1: -1.0, 2: -0.5})
    assert R.decode_graph(lp, 2, g)["frames"].tolist() == [2, 2]            # the final weight decides
    g = DecodingGraph(3, [(0, 1, 1, 0.0), (0, 2, 2, -1.0)], {1: -0.5, 2: 0.0})
    got = R.decode_graph(lp, 2, g)
    assert got["frames"].tolist() == [1, 1] and got["score"] == -0.5
    g = DecodingGraph(2, [(0, 1, 1, -1.0), (0, 1, 1, -0.25)], {1: 0.0})       # parallel arcs, one label: the better weight
    got = R.decode_graph(lp, 2, g)
    assert got["arcs"].tolist() == [1, 1] and got["score"] == -0.25
    g = DecodingGraph(2, [(0, 1, 1, 0.0), (0, 1, 1, 0.0)], {1: 0.0})          # a tie: the lower arc id
    assert R.decode_graph(lp, 2, g)["arcs"].tolist() == [0, 0]


def test_decoding_graph_tables():
    arcs = [(0, 2, 5, -1.0), (0, 1, 3, 0.0), (1, 2, 5, -0.5), (2, 2, 9, 0.0), (1, 1, 3, 0.25), (0, 2, 7, 0.0)]
    g = DecodingGraph(4, arcs, {2: 0.0}, outputs=list("abcdef"))
    assert g.order.tolist() == [1, 4, 0, 2, 3, 5]                             # by dst, the caller's order kept within a node
    assert g.arc_id.tolist() == [2, 0, 3, 4, 1, 5]
    assert g.dst.tolist() == [1, 1, 2, 2, 2, 2] and g.src.tolist() == [0, 1, 0, 1, 2, 0]
    assert g.in_ptr.tolist() == [0, 0, 2, 6, 6]                                # node 3 has no arcs and is unreachable
    assert g.label.tolist() == [3, 3, 5, 5, 9, 7] and g.cols.tolist() == [3, 5, 7, 9] and g.col.tolist() == [0, 0, 1, 1, 3, 2]
    assert g.outputs == list("beacdf") and g.w.dtype == np.float32 and g.w.tolist() == [0.0, 0.25, -1.0, -0.5, 0.0, 0.0]
    assert g.final.tolist() == [-np.inf, -np.inf, 0.0, -np.inf]
    assert [t.dtype for t in g.host_tables()] == [np.int32] * 5 + [np.float32] * 2 + [np.int32]
    assert DecodingGraph(3, arcs[:3], [-np.inf, 0.0, -1.0]).final.tolist() == [-np.inf, 0.0, -1.0]
    with pytest.raises(TypeError):
        g.device_tables("cpu")


def test_decoding_graph_validation():
    ok = [(0, 1, 2, 0.0)]
    for bad in ([(0, 2, 2, 0.0)], [(-1, 1, 2, 0.0)], [(0, 1, 0, 0.0)], [(0, 1, 2, np.inf)], [(0, 1, 2, np.nan)], [(0, 1, 2)], [(0, 1, 1.5, 0.0)]):
        with pytest.raises(ValueError):
            DecodingGraph(2, bad, {1: 0.0})
    for finals in ({2: 0.0}, {1: np.inf}, {1: np.nan}, [0.0], [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError):
            DecodingGraph(2, ok, finals)
    with pytest.raises(ValueError):
        DecodingGraph(0, [], {})
    with pytest.raises(ValueError):
        DecodingGraph(MAX_NODES + 1, ok, {1: 0.0})
    with pytest.raises(ValueError):
        DecodingGraph(2, ok * (MAX_ARCS + 1), {1: 0.0})
    with pytest.raises(ValueError):
        DecodingGraph(2, ok, {1: 0.0}, outputs=["a", "b"])
    assert DecodingGraph(MAX_NODES, ok * MAX_ARCS, {1: 0.0}).num_arcs == MAX_ARCS
    for phrases in ([], [[]], [[1, 2], [1, 2]]):
        with pytest.raises(ValueError):
            DecodingGraph.from_phrases(phrases)
    with pytest.raises(ValueError):
        DecodingGraph.from_phrases([[1], [2]], weights=[0.0])


def test_phrase_trie_shares_prefixes():
    g = DecodingGraph.from_phrases([[1, 2, 3], [1, 2, 4], [1, 5], [1, 2]], weights=[0.0, -1.0, -2.0, -3.0], outputs=list("abcd"))
    # internal: 0 -1-> n1 -2-> n2; the last arcs are the phrases' own: n2 -3-> f, n2 -4-> f, n1 -5-> f, n1 -2-> f
    assert g.num_arcs == 6 and g.num_nodes == 7
    assert sorted(o for o in g.outputs if o is not None) == list("abcd")
    assert sum(np.isfinite(g.final)) == 4 and not np.isfinite(g.final[0])
    by_out = {g.outputs[a]: a for a in range(6) if g.outputs[a] is not None}
    assert [float(g.w[by_out[o]]) for o in "abcd"] == [0.0, -1.0, -2.0, -3.0]
    assert all(np.isfinite(g.final[g.dst[a]]) for a in by_out.values())
    assert g.src[by_out["a"]] == g.src[by_out["b"]] != g.src[by_out["c"]] == g.src[by_out["d"]]
    assert g.accepts([1, 0, 2, 2, 3]) and g.accepts([1, 2]) and g.accepts([1, 5, 0])
    assert not g.accepts([1]) and not g.accepts([1, 2, 3, 1, 5]) and not g.accepts([2]) and not g.accepts([])
    # [1, 2] ends in its own final node: it emits "d" alone
    lp = np.full((2, 6), -8.0)
    lp[0, 1] = lp[1, 2] = 0.0
    got = R.decode_graph(lp, 2, g)
    assert got["frames"].tolist() == [1, 2] and g.outputs[got["trav_arc"][1]] == "d" and got["score"] == -3.0


def test_phrase_loop_returns_to_the_start():
    g = DecodingGraph.from_phrases([[1, 2], [3], [1, 2, 4]], loop=True)
    assert g.num_nodes == 3 and g.num_arcs == 5                               # 0 -1-> n1 -2-> n2 shared; 2, 3 and 4 return to 0
    assert np.isfinite(g.final).tolist() == [True, False, False]
    back = [a for a in range(5) if g.dst[a] == 0]
    assert sorted(g.outputs[a] for a in back) == [0, 1, 2] and sorted(g.label[a] for a in back) == [2, 3, 4]
    assert g.in_ptr.tolist() == [0, 3, 4, 5]
    assert g.accepts([1, 2, 3, 3, 0, 3, 1, 2, 4]) and g.accepts([]) and not g.accepts([1]) and not g.accepts([1, 2, 2, 1])
    lp = np.full((5, 5), -8.0)
    for t, c in enumerate([3, 1, 2, 4, 3]):
        lp[t, c] = 0.0
    got = R.decode_graph(lp, 5, g)
    assert got["score"] == 0.0 and [g.outputs[a] for a in got["trav_arc"][: got["n_trav"]]] == [1, None, None, 2, 1]


def test_from_text_and_linear_and_token_loop():
    t2i = {"a": 1, "b": 2, "c": 3, "_": 0}
    g = DecodingGraph.from_text(["ab c", "", "ab c", "ax", "a_", "b"], t2i, weights=[-1.0, 0, 0, 0, 0, -2.0])
    assert g.skipped == 2 and sorted(o for o in g.outputs if o is not None) == ["abc", "b"]
    assert sorted(g.w.tolist()) == [-2.0, -1.0, 0.0, 0.0]
    g = DecodingGraph.linear([4, 4, 2])
    assert (g.num_nodes, g.src.tolist(), g.dst.tolist(), g.label.tolist()) == (4, [0, 1, 2], [1, 2, 3], [4, 4, 2])
    assert g.final.tolist() == [-np.inf] * 3 + [0.0]
    g = DecodingGraph.token_loop(6)
    assert g.num_nodes == 1 and g.label.tolist() == [1, 2, 3, 4, 5] and g.in_ptr.tolist() == [0, 5] and g.final.tolist() == [0.0]


def test_graph_results_records():
    g = DecodingGraph.from_phrases([[1, 2], [3]], outputs=["one-two", "three"], loop=True)
    a12 = [a for a in range(3) if g.outputs[a] == "one-two"][0]
    a1 = [a for a in range(3) if g.label[a] == 1][0]
    a3 = [a for a in range(3) if g.label[a] == 3][0]
    res = graph_results(g, [-2.0, float("-inf")], [3, 0], [[a1, a12, a3, -1], [-1] * 4], [[1, 3, 6, -1], [-1] * 4],
                        [[2, 4, 6, -1], [-1] * 4], [[-0.5, -1.0, -0.25, 0.0], [0.0] * 4], times=lambda s, e: (s * 0.04, (e + 1) * 0.04))
    assert isinstance(res[0], GraphResult) and res[0].feasible and not res[1].feasible and res[1].tokens == []
    assert res[0].tokens == [1, 2, 3] and res[0].score == -2.0 and not res[0].truncated
    assert [(o["output"], o["start_frame"], o["end_frame"]) for o in res[0].outputs] == [("one-two", 1, 4), ("three", 6, 6)]
    assert res[0].outputs[0]["confidence"] == pytest.approx(np.exp(-1.5 / 4)) and res[0].outputs[0]["end_s"] == pytest.approx(0.2)
    assert res[0].confidences == pytest.approx([np.exp(-0.25), np.exp(-0.5), np.exp(-0.25)])
    assert graph_results(g, [-2.0], [5], [[a1, a12]], [[1, 3]], [[2, 4]], [[-0.5, -1.0]])[0].truncated
