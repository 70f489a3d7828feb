"""CPU: the host builder of the context graph (openeat_amd/utils/context_graph.py) against the brute-force definition of the
yardstick (tests/ctc_bias_beam_ref.py), the yardstick against what is already pinned (with an empty graph it is
ctc_lm_beam_ref.search), a constructed case in which only the biased search keeps the hotword, and the cases the GPU test
runs, shown to be decidable (no two neighbouring totals closer than 1e-8 relative, unless exactly equal)."""
import numpy as np
import pytest

import ctc_bias_beam_ref as BR
import ctc_lm_beam_ref as R
import ngram_ref
from openeat_amd.models.ngram_lm import _EMPTY, _mix_int
from openeat_amd.utils import context_graph
from openeat_amd.utils.context_graph import ContextGraph

GAP_FLOOR = 1e-8          # as tests/test_ctc_lm_beam_ref.py: ten times what the device may differ by

A, B_, C_, D = 1, 2, 3, 4
LONG = tuple(1 + (i * 7 + i // 5) % 5 for i in range(32))
NESTED = [(A, B_), (A, B_, C_), (B_, C_), (B_,), (A, A), (D,), LONG, (C_, A, B_, D), (A, B_, C_, D, 5)]


def _graphs():
    rng = np.random.default_rng(5)
    scores = rng.uniform(-1.0, 4.0, len(NESTED)).astype(np.float32)
    return [(ContextGraph(NESTED, 0.37), BR.make_graph(NESTED, 0.37)),
            (ContextGraph(NESTED, 0.37, scores), BR.make_graph(NESTED, 0.37, scores)),
            (ContextGraph(NESTED[:3], 3.0), BR.make_graph(NESTED[:3], 3.0)),
            (ContextGraph([], 1.5), BR.make_graph([], 1.5))]


def test_walk_equals_the_brute_force_definition():
    rng = np.random.default_rng(11)
    prefixes = [(), (A,), (A, B_), (A, B_, C_), (A, A, A), LONG, LONG[:31], (2,) + LONG + (A, B_), LONG[:20] + LONG]
    prefixes += [tuple(int(t) for t in rng.integers(1, 6, int(rng.integers(1, 45)))) for _ in range(300)]
    prefixes += [tuple(int(t) for t in rng.integers(1, 4, int(rng.integers(1, 20)))) for _ in range(200)]
    for graph, ref in _graphs():
        for p in prefixes:
            for final in (False, True):
                assert graph.bias(p, final) == BR.bias_direct(ref, p, final) == BR.bias(ref, p, final), (p, final)
    graph, ref = _graphs()[0]
    assert graph.bias((A, B_, C_), True) == BR.hits(ref, (A, B_, C_)) > 0.0
    assert BR.pending(ref, LONG[:31]) == 31 and BR.pending(ref, LONG) < 32 and BR.pending(ref, (D,)) == 0
    assert BR.pending(ref, (A, B_, C_)) == 3 and BR.pending(ref, (5, A)) == 1 and BR.pending(ref, (5, 5)) == 0


def _strings(graph):
    """The token string of every state, from the edges."""
    strings = {0: ()}
    for s in range(graph.n_states):                                    # breadth-first numbering: parents first
        for t, nxt in graph._edges[s].items():
            strings[nxt] = strings[s] + (t,)
    return strings


def test_device_tables_decode_back_to_the_automaton():
    for graph, ref in _graphs():
        edges, fail, out, pend = graph.host_tables()
        assert edges.shape == (graph.capacity, 4) and edges.dtype == np.int32 and graph.capacity & (graph.capacity - 1) == 0
        assert fail.shape == pend.shape == (graph.n_states,) and out.shape == (graph.n_states, 2)
        keys = edges[:, :2].copy().view(np.uint64).reshape(-1)
        found = {}
        for slot in np.nonzero(keys != np.uint64(_EMPTY))[0]:
            key = int(keys[slot])
            state, tok = key >> 32, key & 0xFFFFFFFF
            assert (int(slot) - (_mix_int(key) & (graph.capacity - 1))) % graph.capacity <= graph.max_probe
            assert edges[slot, 3] == 0
            found[(state, tok)] = int(edges[slot, 2])
        assert found == {(s, t): n for s in range(graph.n_states) for t, n in graph._edges[s].items()}
        assert len(found) == graph.n_states - 1 and graph.capacity >= 2 * len(found)
        # the states are the distinct prefixes of the phrases; fail / out / pend by their definitions
        strings = _strings(graph)
        node = {v: k for k, v in strings.items()}
        phrases, scores = ref[:2]
        assert set(node) == {q[:i] for q in phrases for i in range(len(q) + 1)} | {()}
        score_of = dict(zip(phrases, scores))
        for s, w in strings.items():
            suffixes = [w[i:] for i in range(1, len(w) + 1) if w[i:] in node]
            assert fail[s] == (node[suffixes[0]] if w else 0), (s, w)
            chain = [w] + suffixes
            assert pend[s] == next((len(x) for x in chain if any(len(q) > len(x) and q[:len(x)] == x for q in phrases)), 0)
            assert out[s, 0:1].view(np.float32)[0] == score_of.get(w, np.float32(0.0)), (s, w)      # 0.0 where no phrase ends
            ending = [x for x in suffixes if x in score_of]
            assert out[s, 1] == (node[ending[0]] if ending else 0), (s, w)


def test_limits_and_duplicates_raise(monkeypatch):
    ContextGraph([tuple(range(1, 33))])
    for bad in ([tuple(range(1, 34))], [()], [(1, 0, 2)], [(1, -3)], [(1, 2), (3,), (1, 2)]):
        with pytest.raises(ValueError):
            ContextGraph(bad)
    for kw in (dict(context_score=float("nan")), dict(context_score=float("inf")), dict(context_score=-0.5),
               dict(phrase_scores=[1.0, float("inf")]), dict(phrase_scores=[1.0])):
        with pytest.raises(ValueError):
            ContextGraph([(1, 2), (3,)], **kw)
    assert context_graph.MAX_STATES == 1 << 20 and context_graph.MAX_PHRASE == 32
    monkeypatch.setattr(context_graph, "MAX_STATES", 6)
    ContextGraph([(1, 2, 3), (1, 2, 4), (5,)])                          # root + 5
    with pytest.raises(ValueError):
        ContextGraph([(1, 2, 3), (1, 2, 4), (5, 6)])


def test_from_text_skips_and_counts_unknown_characters():
    token2id = {"<blank>": 0, "a": 1, "b": 2, "c": 3, "<unk>": 4}
    g = ContextGraph.from_text(["ab c\n", "abz\n", "\n", "abc", "b", "q", " b "], token2id, context_score=2.0)
    assert g.phrases == [(1, 2, 3), (2,)] and g.skipped == 2
    assert g.bias((1, 2, 3), True) == 6.0 + 2.0 and g.bias((1, 2)) == 2.0 + 2.0 * 2


def _lm_case(tmp_path_factory, i):
    Bn, T, V, beam, sharp, order = R.CASES[i]
    logits, lens, path, t2c = R.make_case(tmp_path_factory.mktemp(f"bias{i}"), Bn, T, V, beam, sharp, order)
    return logits, lens, R.PrefixLM(ngram_ref.RefLM(path), t2c), V, beam


@pytest.mark.parametrize("i", [0, 4])
def test_empty_graph_is_the_lm_yardstick(tmp_path_factory, i):
    logits, lens, plm, V, beam = _lm_case(tmp_path_factory, i)
    tp, ti = BR.cpu_topk(logits, beam)
    for graph in (BR.make_graph([], 0.0), BR.make_graph([], 0.37)):
        for lw, lb, eos in ((0.5, 0.0, True), (0.3, 0.8, False)):
            for b in range(len(lens)):
                want, wgap = R.search(tp[b, : lens[b]], ti[b, : lens[b]], beam, plm, lw, lb, eos)
                got, gap = BR.search(tp[b, : lens[b]], ti[b, : lens[b]], beam, graph, plm, lw, lb, eos, final=bool(b % 2))
                assert [h[:4] for h in got] == want and gap == wgap and all(h[4] == 0.0 for h in got)


def test_only_the_biased_search_keeps_the_hotword():
    """Beam 2.  After frame 1 the prefixes are (3,2) -0.4, (3,4) -1.5, (1,2) -2.7, (1,4) -3.8: the plain search cuts (1,2) and
    can never say (1,2,4).  With the phrase [1,2,4] at c = 3 the credit keeps (1) and (1,2) in the beam and the finished
    phrase ends on top with bias 9."""
    tp = [[-0.1, -2.4], [-0.3, -1.4], [-0.2, -1.8]]
    ti = [[3, 1], [2, 4], [4, 0]]
    plain, _ = BR.search(tp, ti, 2, BR.make_graph([], 3.0))
    assert (1, 2, 4) not in [h[0] for h in plain] and plain[0][0] == (3, 2, 4)
    graph = BR.make_graph([(1, 2, 4)], 3.0)
    for final in (True, False):
        got, _ = BR.search(tp, ti, 2, graph, final=final)
        assert got[0][0] == (1, 2, 4) and got[0][4] == 9.0 and got[0][1] == got[0][2] + 9.0, got
    host = ContextGraph([(1, 2, 4)], 3.0)
    assert [host.bias(p) for p in ((1,), (1, 2), (1, 2, 4), (1, 2, 3), (3, 1))] == [3.0, 6.0, 9.0, 0.0, 3.0]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_every_gpu_case_keeps_its_neighbours_apart(tmp_path_factory, i):
    worst = np.inf
    logits, lens, plm, V, beam = _lm_case(tmp_path_factory, i)
    graph = BR.case_graph(logits, lens, V, beam)
    assert len(graph[0]) >= 2
    tp, ti = BR.cpu_topk(logits, beam)
    fired = 0
    for use_lm in (True, False):
        for lw, lb in BR.WEIGHTS:
            for final in (True, False):
                runs = [BR.search(tp[b, : lens[b]], ti[b, : lens[b]], beam, graph, plm if use_lm else None, lw, lb, True, final)
                        for b in range(len(lens))]
                g = min(gap for _, gap in runs)
                fired += sum(h[4] != 0.0 for got, _ in runs for h in got)
                print(f"case {R.CASES[i]} lm {use_lm} weights ({lw}, {lb}) final {final}: smallest non-zero gap {g:.3g}")
                assert g >= GAP_FLOOR, (R.CASES[i], use_lm, lw, lb, final, g)
                worst = min(worst, g)
    assert fired > 0, R.CASES[i]                                    # the graph has something to say in this case
    print(f"smallest gap of all: {worst:.3g}")
