"""CPU: the restatement of the beam-pruned graph decode (ctc_graph_beam_ref.py) against the loop-level restatement of
oe_ctc_graph (ctc_graph_ref.py) where they must agree, its pruning, threshold, last-frame and overflow rules on hand-built
cases, and the host side of large graphs (DecodingGraph(large=), from_arrays, the out-adjacency)."""
import time

import numpy as np
import pytest

import ctc_graph_beam_ref as BR
import ctc_graph_ref as R
from openeat_amd.utils.decoding_graph import BEAM_MAX_ARCS, BEAM_MAX_NODES, MAX_ARCS, MAX_NODES, DecodingGraph, graph_results

NAMES = ("score", "frames", "arcs", "path_logp", "n_trav", "trav_arc", "trav_start", "trav_end", "trav_logp", "n_state", "r_state")


def grid(rng, n, lo):
    return rng.integers(8 * lo, 1, size=n).astype(np.float64) / 8


def random_graph(rng, Q, A, V):
    src = np.where(rng.random(A) < 0.3, rng.integers(0, min(Q, 4), size=A), rng.integers(0, Q, size=A))
    arcs = [(int(s), int(d), int(c), float(w)) for s, d, c, w in zip(src, rng.integers(0, Q, size=A), rng.integers(1, V, size=A), grid(rng, A, -4))]
    finals = {int(q): float(grid(rng, 1, -4)[0]) for q in rng.integers(0, Q, size=max(Q // 2, 1))}
    return DecodingGraph(Q, arcs, finals)


def assert_same(a, b, names=NAMES):
    for k in names:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_beam_equals_the_dense_restatement_on_the_grid(seed, dtype):
    rng = np.random.default_rng(100 + seed)
    Q, A, V, T = int(rng.integers(1, 9)), int(rng.integers(1, 40)), 6, int(rng.integers(1, 14))
    g = random_graph(rng, Q, A, V)
    lp = grid(rng, (T, V), -8)
    for Tb in (T, T // 2, 0):
        want = R.decode_graph(lp, Tb, g, dtype, max_trav=3)
        got = BR.decode_graph(lp, Tb, g, np.inf, None, dtype, max_trav=3)
        assert_same(got, want)
        assert got["status"] == (BR.OK if np.isfinite(want["score"]) else BR.INFEASIBLE)
        assert sum(got["pruned"]) == 0 and got["peak"] <= Q + A
        assert all(np.asarray(got[k]).dtype == np.asarray(want[k]).dtype for k in NAMES)


@pytest.mark.parametrize("beam", [0.0, 1.5, 6.0, np.inf])
def test_float32_equals_float64_on_the_grid(beam):
    rng = np.random.default_rng(7)
    g = random_graph(rng, 12, 60, 6)
    lp = grid(rng, (20, 6), -8)
    a, b = (BR.decode_graph(lp, 20, g, beam, None, dt) for dt in (np.float32, np.float64))
    assert_same(a, b)
    assert (a["status"], a["peak"], a["pruned"], a["survivors"]) == (b["status"], b["peak"], b["pruned"], b["survivors"])


def two_words():
    """0 -1-> 1 -2-> 3 (final) and 0 -3-> 2 -4-> 3: two words of two tokens, weights 0."""
    return DecodingGraph(4, [(0, 1, 1, 0.0), (1, 3, 2, 0.0), (0, 2, 3, 0.0), (2, 3, 4, 0.0)], {3: 0.0})


def test_pruning_drops_what_is_below_the_threshold_and_keeps_what_equals_it():
    g = two_words()
    lp = np.full((4, 5), -8.0)
    lp[0, 1], lp[0, 3] = -1.0, -2.0            # frame 0: arc 0->1 at -1, arc 0->2 at -2, node 0 at -8
    lp[1, 1], lp[1, 3] = -1.0, -1.0
    lp[2:, 2], lp[2:, 4] = -3.0, -0.5          # the second word ends better
    free = BR.decode_graph(lp, 4, g)
    assert free["frames"].tolist() == [3, 3, 4, 4] and free["score"] == -4.0 and sum(free["pruned"]) == 0
    # beam 1: thr_0 = -1 - 1 = -2: the arc at -2 EQUALS it and survives; node 0 (-8) goes
    at = BR.decode_graph(lp, 4, g, beam=1.0)
    assert at["pruned"][0] == 1 and at["frames"].tolist() == [3, 3, 4, 4] and at["score"] == free["score"]
    # beam 0.875: thr_0 = -1.875: the arc at -2 is below it; the second word is lost and the path changes, to a lower score
    below = BR.decode_graph(lp, 4, g, beam=0.875)
    assert below["pruned"][0] == 2 and below["frames"].tolist() == [1, 1, 2, 2] and below["score"] == -8.0 < free["score"]
    assert below["status"] == BR.OK and below["peak"] <= free["peak"]


def test_the_last_frame_is_not_pruned():
    # after the last frame the final state is far below the best state, which is not final: beam 0 must still find it
    g = DecodingGraph(3, [(0, 1, 1, 0.0), (0, 2, 2, 0.0)], {2: 0.0})
    lp = np.array([[-8.0, -0.125, -6.0]])
    out = BR.decode_graph(lp, 1, g, beam=0.0)
    assert out["status"] == BR.OK and out["score"] == -6.0 and out["frames"].tolist() == [2] and out["pruned"] == [0]
    # two frames: frame 0 is pruned, and the same final state is gone: infeasible through pruning alone
    lp2 = np.array([[-8.0, -0.125, -6.0], [-0.125, -0.125, -0.125]])
    assert BR.decode_graph(lp2, 2, g)["status"] == BR.OK
    cut = BR.decode_graph(lp2, 2, g, beam=0.0)
    assert cut["status"] == BR.INFEASIBLE and cut["score"] == -np.inf and (cut["frames"] == -1).all() and cut["pruned"] == [2, 0]
    assert cut["n_trav"] == 0 and (cut["trav_arc"] == -1).all()


def test_overflow_reports_the_first_overflowing_count_and_infeasible_outputs():
    g = two_words()
    lp = np.full((3, 5), -1.0)
    free = BR.decode_graph(lp, 3, g)
    assert free["survivors"] == [3, 7, 8] and free["peak"] == 8 and free["status"] == BR.OK      # 4 nodes + 4 arcs: all alive in the end
    assert BR.decode_graph(lp, 3, g, max_active=8)["status"] == BR.OK                  # exactly max_active decodes
    over = BR.decode_graph(lp, 3, g, max_active=7)
    assert over["status"] == BR.OVERFLOW and over["peak"] == 8 and over["score"] == -np.inf and (over["arcs"] == -1).all()
    first = BR.decode_graph(lp, 3, g, max_active=2)
    assert first["status"] == BR.OVERFLOW and first["peak"] == 3                       # the FIRST overflowing frame's count
    assert BR.decode_graph(lp, 0, g, max_active=1)["status"] == BR.INFEASIBLE and BR.decode_graph(lp, 0, g)["peak"] == 0
    # the last frame counts every reachable state, unpruned
    last = BR.decode_graph(lp, 2, g, beam=0.0, max_active=6)
    assert last["survivors"] == [3, 7] and last["status"] == BR.OVERFLOW and last["peak"] == 7


# ---------------------------------------------------------------- the host side of large graphs
def test_the_default_constructor_keeps_the_dense_limits():
    with pytest.raises(ValueError, match="8064"):
        DecodingGraph(MAX_NODES + 1, [(0, 1, 1, 0.0)], {1: 0.0})
    with pytest.raises(ValueError, match="16384"):
        DecodingGraph(2, [(0, 1, 1, 0.0)] * (MAX_ARCS + 1), {1: 0.0})
    with pytest.raises(ValueError, match="8064"):
        DecodingGraph.from_arrays(MAX_NODES + 1, [0], [1], [1], [0.0], np.zeros(MAX_NODES + 1))
    words = [[1 + i % 50, 1 + i // 50 % 50, 1 + i // 2500] for i in range(20000)]
    with pytest.raises(ValueError):
        DecodingGraph.from_phrases(words)
    with pytest.raises(ValueError):
        DecodingGraph.from_text(["".join(chr(0x4E00 + t) for t in w) for w in words], {chr(0x4E00 + i): i for i in range(1, 60)}, loop=True)
    big = DecodingGraph(MAX_NODES + 1, [(0, 1, 1, 0.0)], {1: 0.0}, large=True)
    assert big.large and big.num_nodes == MAX_NODES + 1 and not DecodingGraph.linear([1]).large
    with pytest.raises(ValueError, match=str(BEAM_MAX_NODES)):
        DecodingGraph.from_arrays(BEAM_MAX_NODES + 1, [0], [1], [1], [0.0], np.zeros(BEAM_MAX_NODES + 1), large=True)
    assert BEAM_MAX_NODES >= 1 << 20 and BEAM_MAX_ARCS >= 1 << 22


def test_large_builders():
    words = [[1 + i % 50, 1 + i // 50 % 50, 1 + i // 2500] for i in range(20000)]
    g = DecodingGraph.from_phrases(words, weights=[-(i % 7) / 8 for i in range(20000)], loop=True, large=True)
    assert g.large and g.num_arcs == 20000 + 2500 + 50 and g.num_nodes == 1 + 50 + 2500 and g.num_arcs > MAX_ARCS
    assert int(np.diff(g.in_ptr)[0]) == 20000 and g.outputs[int(g.arc_id[-1])] == 19999
    t = DecodingGraph.from_text(["".join(chr(0x4E00 + t) for t in w) for w in words], {chr(0x4E00 + i): i for i in range(1, 60)}, loop=True, large=True)
    assert t.num_arcs == g.num_arcs and np.array_equal(t.label, g.label) and t.outputs[int(t.arc_id[-1])] == "".join(chr(0x4E00 + x) for x in words[-1])
    assert g.accepts([1, 0, 1, 1, 0, 1, 0]) and not g.accepts([1, 1, 1])    # word 0 is (1, 1, 1): repeats need a blank between
    res = graph_results(g, [-1.0], [1], [[int(g.arc_id[-1])]], [[0]], [[2]], [[-0.5]])
    assert res[0].feasible and [o["output"] for o in res[0].outputs] == [19999]


def test_from_arrays_equals_the_loop_constructor():
    rng = np.random.default_rng(3)
    Q, A = 50, 400
    src, dst, lab, w = rng.integers(0, Q, A), rng.integers(0, Q, A), rng.integers(1, 9, A), grid(rng, A, -4)
    fin = np.where(rng.random(Q) < 0.5, grid(rng, Q, -2), -np.inf)
    outs = [i if i % 3 else None for i in range(A)]
    a = DecodingGraph(Q, list(zip(src.tolist(), dst.tolist(), lab.tolist(), w.tolist())), fin.tolist(), outs)
    b = DecodingGraph.from_arrays(Q, src, dst, lab, w, fin, outs)
    for k in ("order", "arc_id", "src", "dst", "label", "w", "final", "in_ptr", "cols", "col", "out_ptr", "out_arc"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and np.array_equal(x, y), k
    assert a.outputs == b.outputs and (a.num_nodes, a.num_arcs, a.large) == (b.num_nodes, b.num_arcs, b.large)
    for x, y in zip(a.host_tables() + a.host_out_tables(), b.host_tables() + b.host_out_tables()):
        assert np.array_equal(x, y)
    for bad in (dict(src=src - 1), dict(dst=dst + Q), dict(lab=lab * 0), dict(w=np.where(np.arange(A) == 5, np.inf, w)), dict(src=src[:-1]),
                dict(src=src.astype(np.float64)), dict(fin=fin[:-1]), dict(fin=np.where(np.arange(Q) == 0, np.inf, fin))):
        kw = dict(src=src, dst=dst, lab=lab, w=w, fin=fin) | bad
        with pytest.raises(ValueError):
            DecodingGraph.from_arrays(Q, kw["src"], kw["dst"], kw["lab"], kw["w"], kw["fin"])


def test_the_out_adjacency_lists_every_arc_under_its_source():
    rng = np.random.default_rng(4)
    g = random_graph(rng, 9, 70, 6)
    assert g.out_ptr[0] == 0 and g.out_ptr[-1] == g.num_arcs and sorted(g.out_arc.tolist()) == list(range(g.num_arcs))
    for q in range(g.num_nodes):
        mine = g.out_arc[g.out_ptr[q]: g.out_ptr[q + 1]]
        assert (g.src[mine] == q).all() and (np.diff(mine) > 0).all() and len(mine) == int((g.src == q).sum())


def test_a_million_arcs_build_in_seconds():
    rng = np.random.default_rng(5)
    Q, A = 300_000, 1_000_000
    t0 = time.perf_counter()
    g = DecodingGraph.from_arrays(Q, rng.integers(0, Q, A), rng.integers(0, Q, A), rng.integers(1, 5000, A), -rng.random(A), np.zeros(Q), large=True)
    took = time.perf_counter() - t0
    print(f"from_arrays: {A} arcs in {took:.2f} s")
    assert took < 10 and g.num_arcs == A and (np.diff(g.dst) >= 0).all() and g.out_ptr[-1] == A


def test_the_restatement_is_quick_at_a_hundred_thousand_nodes():
    rng = np.random.default_rng(6)
    Q, A, V, T = 100_000, 250_000, 40, 12
    src = np.where(rng.random(A) < 0.01, 0, rng.integers(0, Q, A))
    g = DecodingGraph.from_arrays(Q, src, rng.integers(0, Q, A), rng.integers(1, V, A), grid(rng, A, -2), np.zeros(Q), large=True)
    lp = grid(rng, (T, V), -8)
    t0 = time.perf_counter()
    free, cut = BR.decode_graph(lp, T, g), BR.decode_graph(lp, T, g, beam=4.0)
    took = time.perf_counter() - t0
    print(f"two decodes of Q={Q} A={A} T={T}: {took:.2f} s, peak {free['peak']} / {cut['peak']}")
    assert took < 30 and free["status"] == BR.OK and sum(cut["pruned"]) > 0 and cut["peak"] < free["peak"] and cut["score"] <= free["score"]
