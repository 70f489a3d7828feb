"""GPU: hotword biasing in the joint CTC/attention beam search - the kernel behind it (oe_context_next) through the C ABI, the
search loop (openeat_amd/utils/joint_search.py) with a table-driven attention scorer against the yardstick
joint_ctx_search_ref.py, and ASRModel.ctc_attention_beam_search with a ContextGraph on the tiny Conformer.

The kernel's states, hits and biases are compared bit for bit with ContextGraph.step / .bias on the host (both add the same
float32 scores in float64 in the same order).  The search is compared with the yardstick exactly in its tokens, order and
finished flags and within 1e-9 * max(1, |x|) in its scores; that is sound because the yardstick's totals and pre-selection
keys keep a distance (asserted here, examined on the host by test_joint_ctx_search_ref.py) far above what the last bit of
an LM term can move.  Every result row's bias is ContextGraph.bias of its tokens to the bit.

The file is not named test_gpu_*: conftest.py orders those files by a fixed list that test_host_logic.py holds complete."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import joint_ctx_search_ref as X  # noqa: E402
import joint_lm_search_ref as R  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402
from openeat_amd.utils import joint_search as js  # noqa: E402
from openeat_amd.utils.context_graph import ContextGraph  # noqa: E402

DEV = "cuda"
SENT, SENT_I = 777.0, -12345
NEG = -math.inf


def bits(t):
    return t.contiguous().view(torch.int64)


def assert_close(got, want, what):
    """-inf exactly where the yardstick has it, the rest within 1e-9 * max(1, |x|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), (what, "-inf pattern", got, want)
    assert not np.isnan(got).any(), (what, "NaN")
    err = np.abs(got[~inf] - want[~inf])
    tol = 1e-9 * np.maximum(1.0, np.abs(want[~inf]))
    assert (err <= tol).all(), (what, float(err.max()) if err.size else 0.0)


def device_graph(graph):
    """The ContextGraph of a ctc_bias_beam_ref graph."""
    phrases, scores, c, _ = graph
    return ContextGraph(phrases, float(c), [float(s) for s in scores])


# ---- the kernel through the C ABI ------------------------------------------------------------------------------------
def raw_next(cg, state, hits, cand, C, eos_tok, want_state=True):
    """-> (out_state (R, C) int32 or None, out_hits (R, C) or None, out_bias (R, C)); every buffer is a row longer than
    (R, C) and prefilled: every entry inside must be written, nothing behind."""
    n = state.shape[0]
    bs = torch.full((n * C + C,), SENT_I, dtype=torch.int32, device=DEV) if want_state else None
    bh = torch.full((n * C + C,), SENT, dtype=torch.float64, device=DEV) if want_state else None
    bb = torch.full((n * C + C,), SENT, dtype=torch.float64, device=DEV)
    hip.check(hip.lib().oe_context_next(hip.context_graph(cg, DEV), hip.ptr(state), hip.ptr(hits), n, hip.ptr(cand), C, eos_tok,
                                        hip.ptr(bs), hip.ptr(bh), hip.ptr(bb), hip.stream()), "oe_context_next")
    torch.cuda.synchronize()
    out = []
    for buf, sent in ((bs, SENT_I), (bh, SENT), (bb, SENT)):
        if buf is None:
            out.append(None)
            continue
        assert (buf[n * C:] == sent).all(), "written behind (R, C)"
        assert not (buf[: n * C] == sent).any(), "an entry of (R, C) was not written"
        out.append(buf[: n * C].view(n, C))
    return out


def host_next(cg, memo, s, h, tok, eos_tok):
    """(state', hits', bias') from ContextGraph.step and the list of ContextGraph.bias, for a hypothesis in (s, h)."""
    if eos_tok >= 0 and tok == eos_tok:
        return s, h, h
    v = memo.get((s, tok))
    if v is None:
        s2 = cg.step(s, tok)
        add, t = [], s2
        while t:
            add.append(float(cg.score[t]))
            t = int(cg.link[t])
        v = memo[s, tok] = (s2, add)
    s2, add = v
    for a in add:
        h = h + a
    return s2, h, h + float(cg.context_score) * int(cg.pend[s2])


def kernel_graphs():
    rng = np.random.default_rng(17)
    nested = [(1, 2, 3), (2, 3), (3,), (2, 3, 4), (5, 4), (5, 4, 1)]          # several phrases end at one position; a prefix of another
    deep = [(1,) * 32, (1, 1, 2), (1, 2)]                                     # 31 ones, then a mismatch: the longest fail walk
    large = sorted({tuple(int(t) for t in rng.integers(1, 259, int(rng.integers(1, 7)))) for _ in range(400)})
    sc = lambda n: rng.uniform(0.1, 2.5, n).astype(np.float32)                # noqa: E731 - sums that are not exact in float32
    graphs = {"nested": ContextGraph(nested, 0.37, sc(len(nested))), "deep": ContextGraph(deep, 0.37, sc(len(deep))),
              "large": ContextGraph(large, 1.3, sc(len(large))), "empty": ContextGraph([], 0.37)}
    assert graphs["large"].max_probe > 0 and graphs["empty"].n_states == 1
    return graphs


def rows_for(cg, name, n, rng):
    """n hypotheses as token prefixes that end inside, at the end of and beside the phrases; -> (prefixes, state, hits) on
    the host, slots r % 4 == 1 missing (state -1, n_states or n_states + 5) for n > 1."""
    prefixes = []
    for r in range(n):
        if name == "deep" and r % 3 == 0:
            p = (1,) * (31 + (r // 3) % 2)
        elif cg.phrases:
            q = cg.phrases[int(rng.integers(0, len(cg.phrases)))]
            p = tuple(int(t) for t in rng.integers(1, 6, int(rng.integers(0, 3)))) + q[: int(rng.integers(0, len(q) + 1))]
        else:
            p = tuple(int(t) for t in rng.integers(1, 6, int(rng.integers(0, 4))))
        prefixes.append(p)
    state, hits = [], []
    for r, p in enumerate(prefixes):
        s = 0
        for t in p:
            s = cg.step(s, t)
        state.append(s)
        hits.append(cg.bias(p, True))
        if n > 1 and r % 4 == 1:
            state[-1] = (-1, cg.n_states, cg.n_states + 5)[(r // 4) % 3]
    return prefixes, state, hits


@pytest.mark.parametrize("name", ["nested", "deep", "large", "empty"])
def test_kernel_bit_for_bit_against_the_host_automaton(name):
    """R in {1, 3, 65} with missing slots, C in {1, 5, 64} and the full-vocabulary form at V in {6, 259}; eos_tok among the
    candidates (a token the phrases use: it must not be walked), outside them and -1; the blank, a negative id and an id beyond
    the vocabulary among the candidates.  State, hits and bias against ContextGraph.step / .bias, the two forms against each
    other, out_bias with the other outputs left out, nothing written outside (R, C)."""
    cg = kernel_graphs()[name]
    rng = np.random.default_rng(5)
    memo = {}
    top = 259 if name == "large" else 6
    for n in (1, 3, 65):
        prefixes, state, hits = rows_for(cg, name, n, rng)
        missing = [not 0 <= s < cg.n_states for s in state]
        assert any(missing) == (n > 1) and not all(missing)
        st_d = torch.tensor(state, dtype=torch.int32, device=DEV)
        h_d = torch.tensor(hits, dtype=torch.float64, device=DEV)

        def check(got, cand, eos_tok, what):
            gs, gh, gb = (None if g is None else g.cpu().numpy() for g in got)
            ws, wh, wb = np.empty(cand.shape, np.int32), np.empty(cand.shape), np.empty(cand.shape)
            for r in range(n):
                for j in range(cand.shape[1]):
                    if missing[r]:
                        ws[r, j], wh[r, j], wb[r, j] = -1, NEG, NEG
                    else:
                        ws[r, j], wh[r, j], wb[r, j] = host_next(cg, memo, state[r], hits[r], int(cand[r, j]), eos_tok)
            assert np.array_equal(gb.view(np.int64), wb.view(np.int64)), (what, "bias")
            if gs is not None:
                assert np.array_equal(gs, ws), (what, "state")
                assert np.array_equal(gh.view(np.int64), wh.view(np.int64)), (what, "hits")
            for r in range(n if n <= 3 else 4):                  # the same through ContextGraph.bias of the whole extended prefix
                for j in range(min(cand.shape[1], 8)):
                    t = int(cand[r, j])
                    if missing[r]:
                        continue
                    if eos_tok >= 0 and t == eos_tok:
                        assert gb[r, j] == cg.bias(prefixes[r], True), (what, r, j)
                    else:
                        assert gb[r, j] == cg.bias(prefixes[r] + (t,), False), (what, r, j)
                        assert gh is None or gh[r, j] == cg.bias(prefixes[r] + (t,), True), (what, r, j)

        for eos_tok in (3 if name != "deep" else 1, 1000, -1):
            fulls = {}
            for V in (6, 259):
                every = np.tile(np.arange(V, dtype=np.int32), (n, 1))
                fulls[V] = raw_next(cg, st_d, h_d, None, V, eos_tok)
                check(fulls[V], every, eos_tok, f"{name} R {n} V {V} eos {eos_tok} full form")
                only = raw_next(cg, st_d, h_d, None, V, eos_tok, want_state=False)
                assert only[0] is None and only[1] is None and torch.equal(bits(only[2]), bits(fulls[V][2]))
            assert torch.equal(bits(fulls[6][2]), bits(fulls[259][2][:, :6])), "the grid shape changed a bit"
            specials = [eos_tok if eos_tok >= 0 else 2, 0, -5, top + 3]
            for C in (1, 5, 64):
                cand = rng.integers(0, top, size=(n, C)).astype(np.int32)
                for r in range(n):
                    for i, t in enumerate(specials):
                        if C == 1:
                            if i == r % len(specials):
                                cand[r, 0] = t
                        else:
                            cand[r, (r + i) % C] = t
                cand_d = torch.from_numpy(cand).to(DEV)
                got = raw_next(cg, st_d, h_d, cand_d, C, eos_tok)
                check(got, cand, eos_tok, f"{name} R {n} C {C} eos {eos_tok}")
                only = raw_next(cg, st_d, h_d, cand_d, C, eos_tok, want_state=False)
                assert torch.equal(bits(only[2]), bits(got[2])), "out_bias changed with out_state / out_hits left out"
                inside = torch.from_numpy((cand >= 0) & (cand < 259)).to(DEV)
                idx = torch.from_numpy(np.clip(cand, 0, 258)).to(DEV).long()
                for k in range(3):
                    shared = fulls[259][k].gather(1, idx)
                    a, b = got[k][inside], shared[inside]
                    assert torch.equal(a, b) if k == 0 else torch.equal(bits(a), bits(b)), "the candidate form and the full form differ"
        # through ops: int64 tensors as the search passes them, both forms
        s3, h3, b3 = ops.context_next(cg, st_d.long(), h_d, cand_d.long(), eos_tok)
        assert torch.equal(s3, got[0]) and torch.equal(bits(h3), bits(got[1])) and torch.equal(bits(b3), bits(got[2]))
        b4 = ops.context_next(cg, st_d.long(), h_d, None, None, V=259, want_state=False)
        assert torch.equal(bits(b4), bits(fulls[259][2]))
        s5, h5, b5 = ops.context_next(cg, st_d, h_d, V=6)
        assert torch.equal(s5, fulls[6][0]) and torch.equal(bits(h5), bits(fulls[6][1])) and torch.equal(bits(b5), bits(fulls[6][2]))


def test_entry_point_and_ops_refuse_what_they_cannot_score():
    cg = kernel_graphs()["nested"]
    state, hits = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    cand = torch.ones(2, 4, dtype=torch.int32, device=DEV)
    out_i = torch.full((8,), SENT_I, dtype=torch.int32, device=DEV)
    out_h, out_b = torch.full((8,), SENT, dtype=torch.float64, device=DEV), torch.full((8,), SENT, dtype=torch.float64, device=DEV)
    lib, g = hip.lib(), hip.context_graph(cg, DEV)

    def call(state=state, hits=hits, n=2, cand=cand, C=4, eos_tok=3, o_s=out_i, o_h=out_h, o_b=out_b):
        return lib.oe_context_next(g, hip.ptr(state), hip.ptr(hits), n, hip.ptr(cand), C, eos_tok, hip.ptr(o_s), hip.ptr(o_h), hip.ptr(o_b),
                                   hip.stream())

    for kw, say in [(dict(state=None), b"null"), (dict(hits=None), b"null"), (dict(o_b=None), b"null"), (dict(o_s=None), b"together"),
                    (dict(o_h=None), b"together"), (dict(n=-1), b"bad shape"), (dict(C=0), b"C must be >= 1"), (dict(eos_tok=-2), b"eos_tok")]:
        assert call(**kw) != 0, kw
        assert say in lib.oe_last_error() and b"oe_context_next" in lib.oe_last_error(), (kw, lib.oe_last_error())
    torch.cuda.synchronize()
    assert (out_i == SENT_I).all() and (out_h == SENT).all() and (out_b == SENT).all(), "a refused call wrote something"
    assert call(n=0) == 0

    with pytest.raises(TypeError, match="CUDA"):
        ops.context_next(cg, state, hits.cpu(), V=6)
    with pytest.raises(TypeError, match="CUDA"):
        ops.context_next(cg, state, hits, cand.cpu())
    with pytest.raises(TypeError, match="integer"):
        ops.context_next(cg, state.float(), hits, V=6)
    with pytest.raises(TypeError, match="float64"):
        ops.context_next(cg, state, hits.float(), V=6)
    with pytest.raises(TypeError, match="integer"):
        ops.context_next(cg, state, hits, cand.float())
    with pytest.raises(TypeError):
        ops.context_next(cg, state, hits, torch.ones(3, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        ops.context_next(cg, state, hits[:1], V=6)
    with pytest.raises(TypeError, match="ContextGraph"):
        ops.context_next("hotwords.txt", state, hits, V=6)
    with pytest.raises(ValueError, match="V"):
        ops.context_next(cg, state, hits)
    with pytest.raises(ValueError):
        ops.context_next(cg, state, hits, V=0)
    with pytest.raises(ValueError):
        ops.context_next(cg, state, hits, torch.ones(2, 0, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="eos"):
        ops.context_next(cg, state, hits, V=6, eos=-2)
    none = ops.context_next(cg, state[:0], hits[:0], V=6)
    assert none[0].shape == (0, 6) and none[2].shape == (0, 6)


# ---- the search loop with a table-driven attention scorer ------------------------------------------------------------
def table_step_fn(table, beam):
    R_, steps = table.shape[0] * beam, table.shape[1] - 1
    utt = torch.arange(R_, device=DEV) // beam

    def step_fn(tokens, parents):
        n = tokens.shape[1]
        last = tokens[:, -1] + 1 if n else torch.zeros(R_, dtype=torch.int64, device=DEV)
        return table[utt, min(n, steps), last].contiguous()
    return step_fn


def compare_search(got, want, cg, with_lm, what):
    names = ((1, "total"), (2, "att"), (3, "ctc")) + (((5, "lm"),) if with_lm else ())
    for u, (nb, (ref_nb, gap, key_gap)) in enumerate(zip(got, want)):
        assert gap >= R.TOTAL_GAP, (what, u, "the yardstick's totals are too close to order", gap)
        assert key_gap >= R.KEY_GAP, (what, u, "the yardstick's pre-selection keys are too close to cut", key_gap)
        assert [h[0] for h in nb] == [h[0] for h in ref_nb], (what, u, nb, ref_nb)
        assert [h[4] for h in nb] == [h[4] for h in ref_nb], (what, u)
        assert all(len(h) == (7 if with_lm else 6) for h in nb), (what, u)
        for k, name in names:
            assert_close([h[k] for h in nb], [h[k] for h in ref_nb], f"{what} utterance {u} {name}")
        for h, rh in zip(nb, ref_nb):
            assert h[-1] == cg.bias(h[0], final=h[4]) == rh[-1], (what, u, h, "bias")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Per shape (and the survivor case) the tables on the host and the device and the graph as (yardstick's, ContextGraph);
    the LM of every (V, order) as (NgramLM, PrefixLM)."""
    tmp = tmp_path_factory.mktemp("joint_ctx")
    tables, graphs, lms = {}, {}, {}
    for name in list(X.SHAPES) + ["survivor"]:
        y, tab, lens = X.make_tables(name)
        tables[name] = (y, tab, lens, torch.from_numpy(y).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
                        torch.from_numpy(tab).to(DEV))
        V = y.shape[2]
        graph = X.survivor_graph(V) if name == "survivor" else X.case_graph(name, y, tab, lens)
        graphs[name] = (graph, device_graph(graph))
        for order in {X.LM_ORDER, R.SURVIVOR["order"], 4}:
            if (V, order) not in lms:
                path, t2c = R.make_lm(tmp, V, order, R.LM_SEED)
                lms[V, order] = (NgramLM(path, t2c), R.prefix_lm(path, t2c))
    return tables, graphs, lms


@pytest.mark.parametrize("beam", R.BEAMS)
@pytest.mark.parametrize("lam", R.LAMS)
@pytest.mark.parametrize("shape", list(X.SHAPES))
def test_search_loop_against_the_yardstick(cases, shape, lam, beam):
    """lm_weight in {0.5, 2.0} (with C = 3, beta = 0 resp. C = 4, beta = 0.5; without an LM the weight only picks C and beta),
    context_prebeam both ways, no LM and an order-2 LM in both lm_prebeam modes; hotwords drawn from the un-biased n-best, so
    that some fire (test_joint_ctx_search_ref.py counts them): n-best lists, their order and the finished flags exactly, total, att, ctc and lm within the bound, bias
    to the bit."""
    tables, graphs, lms = cases
    y, tab, lens, logp, lens_d, table = tables[shape]
    graph, cg = graphs[shape]
    V, Tmax = y.shape[2], y.shape[1]
    ran = 0
    for s, l, b, w, cpre, mode in X.search_cases():
        if (s, l, b) != (shape, lam, beam):
            continue
        C, beta = R.WEIGHTS[w]
        lm, plm, pre = None, None, True
        if mode is not None:
            lm, plm = lms[V, mode[0]]
            pre = mode[1]
        got = js.joint_beam_search(logp, lens_d, table_step_fn(table, beam), beam, C, V - 1, lam, beta, None, 0, lm, w if lm else 0.0, pre,
                                   cg, cpre)
        compare_search(got, X.yardstick(y, tab, lens, graph, plm, beam, C, lam, beta, Tmax, w, pre, cpre), cg, lm is not None,
                       f"{shape} lam={lam} beam={beam} lm_weight={w} context_prebeam={cpre} lm={mode}")
        ran += 1
    assert ran == 12


def zero_graphs():
    return {"empty": ContextGraph([], 0.37), "all zero": ContextGraph([(1, 2), (2,), (3, 1, 2)], 0.0)}


@pytest.mark.parametrize("context_prebeam", [True, False])
@pytest.mark.parametrize("lam", R.LAMS)
@pytest.mark.parametrize("shape", list(X.SHAPES))
def test_empty_and_all_zero_graphs_are_the_search_without_context_by_bit(cases, shape, lam, context_prebeam):
    tables, graphs, lms = cases
    y, tab, lens, logp, lens_d, table = tables[shape]
    V = y.shape[2]
    exact = lambda h: (h[0],) + tuple(np.float64(x).tobytes() for x in h[1:4]) + (h[4],) + tuple(np.float64(x).tobytes() for x in h[5:])  # noqa: E731
    for beam, C, beta in ((1, 3, 0.0), (3, 4, 0.5), (3, V, 0.0)):
        fn = table_step_fn(table, beam)
        for lm_kw in ((), (lms[V, 4][0], 0.7, True), (lms[V, 4][0], 0.7, False)):
            want = js.joint_beam_search(logp, lens_d, fn, beam, C, V - 1, lam, beta, None, 0, *lm_kw)
            assert sum(len(nb) for nb in want) > 0
            for name, cg in zero_graphs().items():
                got = js.joint_beam_search(logp, lens_d, fn, beam, C, V - 1, lam, beta, None, 0, *lm_kw, context=cg,
                                           context_prebeam=context_prebeam)
                assert [[exact(h[:-1]) for h in nb] for nb in got] == [[exact(h) for h in nb] for nb in want], (name, lam, beam, lm_kw[1:])
                assert all(h[-1] == 0.0 and len(h) == len(w) + 1 for nb, wb in zip(got, want) for h, w in zip(nb, wb))


@pytest.mark.parametrize("context_prebeam", [True, False])
def test_a_finished_hypothesis_keeps_its_bias_while_it_waits(cases, context_prebeam):
    """<eos> is likely at the first step and all but impossible afterwards, and every token is a hotword of its own: the
    hypothesis that ended at once keeps its slot, its scores and its bias - 0, the empty prefix - step after step, while the
    other slots go on growing and collect a score with every token."""
    c = R.SURVIVOR
    tables, graphs, lms = cases
    y, tab, lens, logp, lens_d, table = tables["survivor"]
    graph, cg = graphs["survivor"]
    lm, plm = lms[c["V"], c["order"]]
    first = None
    for max_steps in (1, 2, 3, 4, 5):
        got = js.joint_beam_search(logp, lens_d, table_step_fn(table, c["beam"]), c["beam"], c["C"], c["V"] - 1, c["lam"], 0.0, max_steps,
                                   0, lm, c["lm_weight"], True, cg, context_prebeam)
        compare_search(got, X.yardstick(y, tab, lens, graph, plm, c["beam"], c["C"], c["lam"], 0.0, max_steps, c["lm_weight"], True,
                                        context_prebeam), cg, True, f"max_steps={max_steps}")
        for nb in got:
            assert [h[4] for h in nb] == [True, False, False] and nb[0][0] == [] and nb[0][6] == 0.0, nb
            assert all(len(h[0]) == max_steps and h[6] > 0 for h in nb[1:]), nb
        first = first or [nb[0] for nb in got]
        assert [nb[0] for nb in got] == first, "the finished hypothesis changed while it waited"


@pytest.mark.parametrize("context_prebeam", [True, False])
def test_one_step_with_the_graph_is_capturable(cases, context_prebeam):
    """Score + prune of one step with the graph under torch.cuda.graph, replayed twice: the bits of the eager step."""
    tables, graphs, lms = cases
    y, tab, lens, logp, lens_d, table = tables["mid"]
    V = y.shape[2]
    cg = device_graph(X.survivor_graph(V))                       # every token is a hotword: a row that holds a token has a bias
    beam, C, lam, beta = 3, 5, 0.3, 0.5
    fn = table_step_fn(table, beam)
    kw = dict(context=cg, context_prebeam=context_prebeam)
    st = js.initial_state(logp, lens_d, beam, lam, 0, None, cg, context_prebeam)
    for _ in range(2):
        st = js.search_step(logp, lens_d, st, fn(st.tokens, st.parents), beam, C, V - 1, lam, beta, 0, None, **kw)
    att_logp = fn(st.tokens, st.parents)
    eager = js.search_step(logp, lens_d, st, att_logp, beam, C, V - 1, lam, beta, 0, None, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = js.search_step(logp, lens_d, st, att_logp, beam, C, V - 1, lam, beta, 0, None, **kw)
    for _ in range(2):
        for t in (out.tokens, out.total, out.att, out.ctc, out.cstate, out.hits, out.bias):
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        alive = (eager.total > NEG).cpu()
        growing = (eager.total > NEG) & (eager.length > 0)        # the hypothesis that ended at once holds no token: bias 0
        assert growing.any() and (eager.bias[growing] != 0).all()
        assert torch.equal(out.tokens.cpu()[alive], eager.tokens.cpu()[alive])
        assert torch.equal(out.parents, eager.parents) and torch.equal(out.finished, eager.finished)
        assert torch.equal(out.cstate, eager.cstate)
        for a, b in ((out.total, eager.total), (out.att, eager.att), (out.ctc, eager.ctc), (out.hits, eager.hits), (out.bias, eager.bias)):
            assert torch.equal(bits(a), bits(b))


# ---- end to end on the tiny Conformer --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), g["in"]["feats"][:2].contiguous().to(DEV), g["in"]["flen"][:2].to(DEV), meta


KW = dict(beam_size=3, ctc_weight=0.3, nbest=True, max_len=8)


@pytest.mark.parametrize("context_prebeam", [True, False])
def test_model_all_zero_graph_is_the_search_without_context(tiny_conformer, context_prebeam):
    model, feats, flen, meta = tiny_conformer
    want = model.ctc_attention_beam_search(feats, flen, **KW)
    cg = ContextGraph([(1, 2), (3,), (4, 5, 6)], 0.0)
    got = model.ctc_attention_beam_search(feats, flen, context=cg, context_prebeam=context_prebeam, **KW)
    exact = lambda h: (h[0],) + tuple(np.float64(x).tobytes() for x in h[1:4])                            # noqa: E731
    assert [[exact(h) for h in nb] for nb in got] == [[exact(h) for h in nb] for nb in want]
    assert all(len(h) == 5 and h[4] == 0.0 for nb in got for h in nb) and all(len(h) == 4 for nb in want for h in nb)
    kw = dict(KW, nbest=False)
    assert model.ctc_attention_beam_search(feats, flen, context=cg, context_prebeam=context_prebeam, **kw) == [nb[0][0] for nb in want]


def contains(tokens, q):
    return any(tuple(tokens[i:i + len(q)]) == tuple(q) for i in range(len(tokens) - len(q) + 1))


@pytest.mark.parametrize("context_prebeam", [True, False])
def test_model_a_hotword_lifts_the_second_best_and_rows_carry_their_bias(tiny_conformer, context_prebeam):
    """The hotword is the token sequence of a lower-ranked hypothesis of the un-biased search that the best one does not
    contain; with a score far above the distance between the two, the best hypothesis of the biased search contains it.
    Every row's bias is ContextGraph.bias of its tokens (finished: the credit dropped; the list does not say which) and its
    total recomposes from att, ctc, length and bias."""
    model, feats, flen, meta = tiny_conformer
    lam, beta, score = 0.3, 0.25, 40.0
    kw = dict(KW, ctc_weight=lam, length_bonus=beta)
    want = model.ctc_attention_beam_search(feats, flen, **kw)
    lifted = 0
    for u, nb in enumerate(want):
        picks = [h[0] for h in nb[1:] if h[0] and not contains(nb[0][0], h[0])]
        if not picks:
            continue
        q = tuple(picks[0])
        cg = ContextGraph([q], 0.5, [score])
        got = model.ctc_attention_beam_search(feats, flen, context=cg, context_prebeam=context_prebeam, **kw)
        assert contains(got[u][0][0], q) and not contains(want[u][0][0], q), (u, q, got[u], want[u])
        assert got[u][0][4] >= score
        assert model.ctc_attention_beam_search(feats, flen, context=cg, context_prebeam=context_prebeam, **dict(kw, nbest=False)) == \
            [g[0][0] for g in got]
        for gb in got:
            for tokens, total, att, ctc, b in gb:
                assert b in (cg.bias(tokens, final=False), cg.bias(tokens, final=True)), (tokens, b)
                mix = (((1 - lam) * att + lam * ctc) + beta * len(tokens)) + b
                assert abs(total - mix) <= 1e-9 * max(1.0, abs(mix)), (tokens, total, mix)
        lifted += 1
    assert lifted > 0, "no utterance has a lower-ranked hypothesis the best one does not contain"


def test_model_refuses_a_graph_it_cannot_use(tiny_conformer):
    model, feats, flen, meta = tiny_conformer
    V = meta["V"]
    for context in ([(1, 2)], "hotwords.txt", ContextGraph([(1, V)]), ContextGraph([(2,), (1, V + 7, 3)]), ContextGraph([(1, model.eos)])):
        with pytest.raises(ValueError):
            model.ctc_attention_beam_search(feats, flen, beam_size=2, context=context)
    logp = torch.zeros(1, 2, V, device=DEV)
    with pytest.raises(ValueError, match="ContextGraph"):
        js.joint_beam_search(logp, None, lambda t, p: logp[:, 0], 1, 2, V - 1, context=object())
