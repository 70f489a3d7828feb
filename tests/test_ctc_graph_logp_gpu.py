"""GPU: the graph CTC likelihood and its gradient (oe_ctc_graph_logp / oe_ctc_graph_logp_grad) through the C ABI against the
float64 restatement (ctc_graph_logp_ref.py), and through ops.ctc_graph_logp / ASRModel.ctc_graph_loss / ctc_graph_search.

Tolerances: the ones include/openeat_hip.h states for oe_ctc_loss_fused - logp rtol 1e-4 / atol 1e-3, gradient rtol 2e-3 /
atol 2e-5 * |g[b]| - against the float64 restatement.  Every comparison prints the worst fraction of its tolerance it used
(`-s` shows them; DESIGN.md records the measured ones).

The kernel runs 1024 threads per utterance, gives a node of more than 32 arcs (in for alpha, out for beta) and a column of more
than 32 arcs to a wave, and loads a thread's first lp one frame ahead: the token loops (one node, V - 1 groups), the looped
trie (groups of several arcs, out-arcs whose label matches an in-group) and the graph at the limits cover those paths.

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_graph_logp_ref as R  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.utils.decoding_graph import LOGP_MAX_ARCS, LOGP_MAX_NODES, DecodingGraph, GraphSet  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3
G_RTOL, G_ATOL = 2e-3, 2e-5
SENT = 5.0


class Call:
    """oe_ctc_graph_logp and oe_ctc_graph_logp_grad on one batch, sentinel-filled outputs; the columns behind V hold 3.0."""

    def __init__(self, logits, hlens, graphs, graph_of=None, g=None, normalized=False, ldv=None):
        logits = torch.as_tensor(np.asarray(logits), dtype=torch.float32)
        self.B, self.T, self.V = (int(s) for s in logits.shape)
        self.ldv = ldv or self.V
        self.buf = torch.full((self.B, self.T, self.ldv), 3.0, device=DEV)
        self.buf[:, :, :self.V] = logits.to(DEV)
        self.gset = graphs if isinstance(graphs, GraphSet) else GraphSet(graphs)
        self.set = hip.graph_set(self.gset, DEV)
        self.hl = torch.as_tensor(np.asarray(hlens), dtype=torch.int32).to(DEV)
        self.graph_of = None if graph_of is None else torch.as_tensor(np.asarray(graph_of), dtype=torch.int32).to(DEV)
        self.g = torch.as_tensor(np.ones(self.B) if g is None else np.asarray(g), dtype=torch.float32).to(DEV)
        self.normalized = int(normalized)
        lib = hip.lib()
        U = len(self.gset.cols)
        self.ws = torch.empty(max(lib.oe_ctc_graph_logp_workspace_bytes(self.B, self.T, U, self.gset.Qmax, self.gset.Amax), 16),
                              dtype=torch.uint8, device=DEV)
        self.gws = torch.empty(max(lib.oe_ctc_graph_logp_grad_workspace_bytes(self.B, self.T, U, self.gset.Qmax, self.gset.Amax), 16),
                               dtype=torch.uint8, device=DEV)
        self.fresh()

    def fresh(self):
        self.logp = torch.full((self.B,), SENT, device=DEV)
        self.logp2 = torch.full((self.B,), SENT, device=DEV)
        self.dl = torch.full((self.B, self.T, self.ldv), SENT, device=DEV)

    def score_args(self):
        a = hip.CtcGraphLogpArgs()
        a.logits, a.ldv, a.B, a.T, a.V = self.buf.data_ptr(), self.ldv, self.B, self.T, self.V
        a.hlens, a.set = self.hl.data_ptr(), C.pointer(self.set)
        a.graph_of = None if self.graph_of is None else self.graph_of.data_ptr()
        a.normalized, a.logp, a.workspace = self.normalized, self.logp.data_ptr(), self.ws.data_ptr()
        return a

    def grad_args(self):
        a = hip.CtcGraphLogpGradArgs()
        a.logits, a.ldv, a.B, a.T, a.V = self.buf.data_ptr(), self.ldv, self.B, self.T, self.V
        a.hlens, a.set = self.hl.data_ptr(), C.pointer(self.set)
        a.graph_of = None if self.graph_of is None else self.graph_of.data_ptr()
        a.normalized, a.g, a.dlogits, a.logp, a.workspace = self.normalized, self.g.data_ptr(), self.dl.data_ptr(), self.logp2.data_ptr(), \
            self.gws.data_ptr()
        return a

    def score(self, a=None):
        return hip.lib().oe_ctc_graph_logp(C.byref(a or self.score_args()), hip.stream())

    def grad(self, a=None):
        return hip.lib().oe_ctc_graph_logp_grad(C.byref(a or self.grad_args()), hip.stream())

    def run(self, grad=True):
        hip.check(self.score(), "oe_ctc_graph_logp")
        if grad:
            hip.check(self.grad(), "oe_ctc_graph_logp_grad")
        torch.cuda.synchronize()
        return self

    def untouched(self):
        return bool((self.logp == SENT).all() and (self.logp2 == SENT).all() and (self.dl == SENT).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def check_logp(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf]), (what, got, want)          # -inf exactly
    frac = np.abs(got[~inf] - want[~inf]) / (ATOL + RTOL * np.abs(want[~inf]))
    worst = float(frac.max()) if frac.size else 0.0
    print(f"FRACTION logp {what}: {worst:.4f}")
    assert worst <= 1.0, (what, got, want)
    return worst


def check_grad(got, want, g, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = G_ATOL * np.abs(np.asarray(g, dtype=np.float64))[:, None, None] + G_RTOL * np.abs(want)
    tol = np.where(np.isfinite(tol), tol, 0.0)                              # g = NaN: an infeasible utterance, exact zeros
    err = np.abs(got - want)
    worst = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))))
    print(f"FRACTION grad {what}: {worst:.4f}")
    assert worst <= 1.0, what
    return worst


def against_ref(call, graphs, graph_of, logits, hlens, g, what, normalized=False):
    want_lp, want_dl = R.logp_and_grad(logits, hlens, graphs, graph_of, g=np.nan_to_num(np.asarray(g, dtype=np.float64)), normalized=normalized)
    check_logp(call.logp.cpu().numpy(), want_lp, what)
    if not normalized:
        assert np.array_equal(bits(call.logp), bits(call.logp2)), what      # the two entries agree in every bit
        check_grad(call.dl[:, :, :call.V].cpu().numpy(), want_dl, g, what)
    return want_lp, want_dl


# ---------------------------------------------------------------- 1, 9: random graphs ----
@functools.lru_cache(maxsize=None)
def case1():
    rng = np.random.default_rng(101)
    B, T, V = 5, 23, 9
    graphs = [R.random_graph(rng, int(rng.integers(3, 13)), int(rng.integers(8, 41)), V, final_p=0.5) for _ in range(4)]
    graphs.append(DecodingGraph(4, [(0, 1, 2, 0.0), (1, 1, 3, -0.5), (2, 3, 1, 0.0)], {3: 0.0}))     # its final node is unreachable
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    hlens = np.array([T, 0, 17, 9, T], dtype=np.int32)
    g = np.array([1.0, -0.5, 2.5, 0.75, np.nan], dtype=np.float32)
    call = Call(logits, hlens, graphs, graph_of=np.arange(B), g=g, ldv=V + 3).run()
    return graphs, logits, hlens, g, call


def test_random_graphs():
    graphs, logits, hlens, g, call = case1()
    B, T, V = logits.shape
    want_lp, _ = against_ref(call, graphs, np.arange(B), logits, hlens, g, "random graphs")
    assert np.isfinite(want_lp[[0, 2, 3]]).all() and want_lp[1] == -np.inf and want_lp[4] == -np.inf
    dl = call.dl.cpu().numpy()
    assert (dl[:, :, V:] == SENT).all()                                     # columns >= V are never written
    assert not dl[4, :, :V].any() and not dl[1, :, :V].any()                # infeasible (g = NaN) and Tb = 0: exact zeros
    for b in range(B):
        assert not dl[b, hlens[b]:, :V].any()
    assert np.isfinite(dl[:, :, :V]).all()


def test_relation_to_the_best_path():
    graphs, logits, hlens, g, call = case1()
    lg, hl = torch.from_numpy(logits).to(DEV), torch.from_numpy(hlens).to(DEV)
    logp = call.logp.cpu().numpy()
    for b, gr in enumerate(graphs):
        score = float(ops.ctc_graph_decode(lg[b:b + 1], hl[b:b + 1], gr)[0][0])
        assert (score == -np.inf) == (logp[b] == -np.inf)
        if np.isfinite(score):
            assert logp[b] >= score - ATOL, (b, logp[b], score)
    # near-one-hot posteriors: the best path carries the whole mass
    rng = np.random.default_rng(9)
    gr = DecodingGraph.from_phrases([[1, 2, 3], [1, 4], [2, 2, 5], [5]], weights=[-0.5, -1.0, 0.0, -2.0])
    frames = [0, 2, 2, 0, 2, 5, 5, 0]
    lp = -50.0 - 10.0 * rng.random(size=(1, len(frames), 7))
    lp[0, np.arange(len(frames)), frames] = 0.0
    c = Call(lp, [len(frames)], [gr], normalized=True).run(grad=False)
    score = float(ops.ctc_graph_decode(torch.from_numpy(lp.astype(np.float32)).to(DEV), c.hl, gr, normalized=True)[0][0])
    assert score == 0.0 and abs(float(c.logp[0]) - score) <= ATOL


# ---------------------------------------------------------------- 2: linear chains ----
def test_linear_chains_against_the_nbest_scorer():
    rng = np.random.default_rng(23)
    B, T, V = 3, 31, 11
    toks = [[4, 4, 7, 1, 1, 1, 9], [3], [2, 5, 5, 2, 2, 10, 6, 6]]
    graphs = [DecodingGraph.linear(t) for t in toks]
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    hlens = np.array([T, 12, 27], dtype=np.int32)
    g = np.array([1.0, -2.0, 0.5], dtype=np.float32)
    call = Call(logits, hlens, graphs, graph_of=[0, 1, 2], g=g).run()
    against_ref(call, graphs, [0, 1, 2], logits, hlens, g, "linear chains")
    hyps = torch.zeros(B, 8, dtype=torch.int32)
    for b, t in enumerate(toks):
        hyps[b, :len(t)] = torch.tensor(t, dtype=torch.int32)
    x = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    nb = ops.ctc_nbest_logp(x, call.hl, hyps.to(DEV), torch.tensor([len(t) for t in toks], dtype=torch.int32, device=DEV), 1).view(B)
    (nb * call.g).sum().backward()
    check_logp(call.logp.cpu().numpy(), nb.detach().cpu().numpy(), "linear chains vs oe_ctc_nbest_score")
    check_grad(call.dl.cpu().numpy(), x.grad.cpu().numpy(), g, "linear chains vs oe_ctc_nbest_grad")


# ---------------------------------------------------------------- 3: token loops ----
@pytest.mark.parametrize("V,T", [(300, 19), (3246, 8)])
def test_token_loops(V, T):
    rng = np.random.default_rng(V)
    B = 2
    logits = (rng.normal(size=(B, T, V)) * 3.0).astype(np.float32)
    logits[1, :, 5] += 12.0                                                  # a peaky utterance beside a flat one
    g = np.array([1.5, -2.0], dtype=np.float32)
    call = Call(logits, [T, T - 3], [DecodingGraph.token_loop(V)], g=g).run()
    logp, dl = call.logp.cpu().numpy(), call.dl.cpu().numpy()
    print(f"FRACTION logp token loop V={V}: {np.abs(logp).max() / ATOL:.4f}")
    print(f"FRACTION grad token loop V={V}: {(np.abs(dl) / (G_ATOL * np.abs(g))[:, None, None]).max():.4f}")
    assert np.array_equal(bits(call.logp), bits(call.logp2))
    assert (np.abs(logp) <= ATOL).all(), logp
    assert (np.abs(dl) <= (G_ATOL * np.abs(g))[:, None, None]).all()


# ---------------------------------------------------------------- 4: looped trie ----
def test_looped_trie():
    rng = np.random.default_rng(41)
    V, T, B = 14, 40, 2
    phrases = set()
    while len(phrases) < 50:
        n = int(rng.integers(1, 5))
        phrases.add(tuple(int(x) for x in rng.integers(1, V, size=n - 1)) + (int(rng.choice([3, 3, 7, 7, int(rng.integers(1, V))])),))
    phrases = sorted(phrases)
    gr = DecodingGraph.from_phrases(phrases, weights=[-0.1 * (i % 7) for i in range(len(phrases))], loop=True)
    t = GraphSet([gr]).graph_tables(0)
    sizes = np.diff(t["in_gstart"][t["in_gptr"][0]:t["in_gptr"][1] + 1])
    assert sizes.max() > 1 and (t["in_xg"] >= 0).any()                       # groups of several arcs; out-arcs matching an in-group
    logits = (rng.normal(size=(B, T, V)) * 1.5).astype(np.float32)
    hlens, g = np.array([T, 33], dtype=np.int32), np.array([1.0, -1.25], dtype=np.float32)
    call = Call(logits, hlens, [gr], g=g).run()
    want_lp, _ = against_ref(call, [gr], None, logits, hlens, g, "looped trie")
    assert np.isfinite(want_lp).all()


# ---------------------------------------------------------------- 5: cancellation ----
def cells(n):
    arcs = []
    for i in range(n):
        arcs += [(2 * i, 2 * i + 1, 1, 0.0), (2 * i, 2 * i + 1, 2, 0.0), (2 * i + 1, 2 * i + 2, 1, 0.0)]
    return DecodingGraph(2 * n + 1, arcs, {2 * n: 0.0})


def test_exclusion_does_not_cancel():
    row = np.array([-100.0, 0.0, -40.0])
    lp = np.tile(row, (1, 3, 1))
    call = Call(lp, [3], [cells(1)], normalized=True).run(grad=False)
    got = float(call.logp[0])
    print(f"cancellation cell: logp = {got!r} (the path 2,1,1 carries -40)")
    check_logp([got], [-40.0], "cancellation cell vs -40")
    check_logp([got], R.logp_and_grad(lp, [3], cells(1), normalized=True)[0], "cancellation cell")
    lp = np.tile(row, (1, 60, 1))
    gr = cells(20)
    call = Call(lp, [60], [gr], normalized=True).run(grad=False)
    check_logp(call.logp.cpu().numpy(), R.logp_and_grad(lp, [60], gr, normalized=True)[0], "cancellation chain of 20")


# ---------------------------------------------------------------- 6: at the limits ----
def wide_dag(rng, Q, A, V):
    arcs = [(0, 1, 1, 0.0), (int(rng.integers(0, 2)), 2, 2, 0.0)]
    arcs += [(int(rng.integers(0, 3)), q, int(rng.integers(1, V)), float(rng.normal() * 0.3)) for q in range(3, Q)]
    arcs += [(int(rng.integers(0, 40)), Q - 1, int(rng.integers(1, 6)), 0.0) for _ in range(40)]     # a node of many incoming arcs
    while len(arcs) < A:
        s = int(rng.integers(0, Q - 1))
        arcs.append((s, int(rng.integers(s + 1, Q)), int(rng.integers(1, V)), float(rng.normal() * 0.3)))
    return DecodingGraph(Q, arcs, {int(q): 0.0 for q in rng.choice(Q, size=Q // 3, replace=False)})


def test_at_the_limits():
    rng = np.random.default_rng(61)
    V, T = 50, 4
    gr = wide_dag(rng, LOGP_MAX_NODES, LOGP_MAX_ARCS, V)
    assert (gr.num_nodes, gr.num_arcs) == (LOGP_MAX_NODES, LOGP_MAX_ARCS) and LOGP_MAX_NODES >= 2048 and LOGP_MAX_ARCS >= 4096
    logits = (rng.normal(size=(2, T, V)) * 2.0).astype(np.float32)
    hlens, g = np.array([T, 3], dtype=np.int32), np.array([1.0, 2.0], dtype=np.float32)
    call = Call(logits, hlens, [gr], g=g).run()
    want_lp, _ = against_ref(call, [gr], None, logits, hlens, g, "at the limits")
    assert np.isfinite(want_lp).all()
    lib = hip.lib()
    U = len(gr.cols)
    for fn in (lib.oe_ctc_graph_logp_workspace_bytes, lib.oe_ctc_graph_logp_grad_workspace_bytes):
        assert fn(2, T, U, LOGP_MAX_NODES, LOGP_MAX_ARCS) > 0
        assert fn(2, T, U, LOGP_MAX_NODES + 1, LOGP_MAX_ARCS) == 0 and fn(2, T, U, LOGP_MAX_NODES, LOGP_MAX_ARCS + 1) == 0
        assert fn(2, 0, U, 8, 8) == 0 and fn(2, (1 << 20) + 1, U, 8, 8) == 0 and fn(0, T, U, 8, 8) == 0
    for field, limit in (("Qmax", LOGP_MAX_NODES), ("Amax", LOGP_MAX_ARCS)):
        call.fresh()
        setattr(call.set, field, limit + 1)                                  # one over: reported, nothing launched
        assert call.score() != 0 and field.encode() in lib.oe_last_error()
        assert call.grad() != 0 and field.encode() in lib.oe_last_error()
        torch.cuda.synchronize()
        assert call.untouched()
        setattr(call.set, field, limit)
    with pytest.raises(ValueError):
        GraphSet([DecodingGraph(LOGP_MAX_NODES + 1, [(0, 1, 1, 0.0)], {1: 0.0})])


# ---------------------------------------------------------------- 7: long utterance ----
def test_long_utterance():
    rng = np.random.default_rng(71)
    V, T = 40, 600
    segments = []
    for i in range(120):
        kind = i % 4
        if kind == 1:
            segments.append([[int(rng.integers(1, V))], [int(rng.integers(1, V)), int(rng.integers(1, V))]])     # two spellings
        elif i % 24 == 6:
            segments.append([[int(rng.integers(1, V))], []])                # an optional filler
        else:
            segments.append([[int(rng.integers(1, V))]])
    gr = DecodingGraph.from_alternatives(segments)
    assert sum(len(s) == 2 and all(s) for s in segments) == 30 and gr.num_arcs >= 150
    logits = (rng.normal(size=(1, T, V)) * 0.5).astype(np.float32)          # untrained-like: nearly flat posteriors
    g = np.array([1.0], dtype=np.float32)
    call = Call(logits, [T], [gr], g=g).run()
    want_lp, _ = against_ref(call, [gr], None, logits, [T], g, "long utterance T=600")
    assert want_lp[0] < -1000.0                                             # where a float32 trellis drifts


# ---------------------------------------------------------------- 8: a graph set ----
def test_graph_set_groups_and_repeatability():
    rng = np.random.default_rng(81)
    B, T, V = 4, 21, 12
    graphs = [DecodingGraph.from_phrases([[1, 2], [3, 2, 2], [4]], loop=True), R.random_graph(rng, 9, 30, V, final_p=0.6),
              DecodingGraph.linear([5, 5, 6, 7, 1, 11, 2, 8, 9, 10])]
    graph_of = [2, 0, 1, 0]
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    hlens, g = np.array([T, 15, T, 20], dtype=np.int32), np.array([1.0, 0.5, -1.0, 2.0], dtype=np.float32)
    call = Call(logits, hlens, graphs, graph_of=graph_of, g=g).run()
    lp, lp2, dl = bits(call.logp), bits(call.logp2), bits(call.dl)
    assert np.array_equal(lp, lp2) and np.isfinite(call.logp.cpu().numpy()).all()
    call.fresh()
    call.run()
    assert np.array_equal(lp, bits(call.logp)) and np.array_equal(dl, bits(call.dl))            # run to run
    for gi in range(3):                                                     # three single-graph calls on the same utterances
        idx = [b for b in range(B) if graph_of[b] == gi]
        one = Call(logits[idx], hlens[idx], [graphs[gi]], g=g[idx]).run()
        assert np.array_equal(bits(one.logp), lp[idx]) and np.array_equal(bits(one.dl), dl[idx]), gi
    x = torch.from_numpy(logits).to(DEV)
    outs = []
    for cap in (1 << 30, 1):                                                # one call; groups of one utterance
        xi = x.clone().requires_grad_(True)
        out = ops.ctc_graph_logp(xi, call.hl, graphs, graph_of, workspace_cap=cap)
        (out * call.g).sum().backward()
        outs.append((bits(out), bits(xi.grad)))
    assert np.array_equal(outs[0][0], lp) and np.array_equal(outs[1][0], lp)
    assert np.array_equal(outs[0][1], dl) and np.array_equal(outs[1][1], dl)


# ---------------------------------------------------------------- 10: capture ----
def test_graph_capture():
    rng = np.random.default_rng(91)
    B, T, V = 3, 17, 10
    graphs = [R.random_graph(rng, 8, 25, V, final_p=0.6), DecodingGraph.token_loop(V)]
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    call = Call(logits, [T, 11, T], graphs, graph_of=[0, 1, 0], g=[1.0, 2.0, -1.0]).run()
    eager = (bits(call.logp), bits(call.logp2), bits(call.dl))
    sa, ga = call.score_args(), call.grad_args()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            hip.check(call.score(sa), "oe_ctc_graph_logp")
            hip.check(call.grad(ga), "oe_ctc_graph_logp_grad")
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for _ in range(2):
        for t in (call.logp, call.logp2, call.dl):
            t.fill_(SENT)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((bits(call.logp), bits(call.logp2), bits(call.dl)), eager):
            assert np.array_equal(got, want)


# ---------------------------------------------------------------- 11: bad arguments ----
def test_bad_arguments_are_reported_not_launched():
    rng = np.random.default_rng(5)
    B, T, V = 2, 6, 7
    logits = rng.normal(size=(B, T, V)).astype(np.float32)
    call = Call(logits, [T, T], [DecodingGraph.linear([1, 2])], ldv=V + 1)
    lib = hip.lib()

    def rejected(fn, a, word):
        rc = fn(a)
        torch.cuda.synchronize()
        assert rc != 0 and word in lib.oe_last_error().decode(), (word, lib.oe_last_error())
        assert call.untouched()

    for field in ("logits", "hlens", "logp", "workspace", "set"):
        a = call.score_args()
        setattr(a, field, None)
        rejected(call.score, a, "null")
    for field in ("logits", "hlens", "g", "dlogits", "workspace", "set"):
        a = call.grad_args()
        setattr(a, field, None)
        rejected(call.grad, a, "null")
    a = call.grad_args()
    a.logp = None                                                           # optional: not an error
    hip.check(call.grad(a), "oe_ctc_graph_logp_grad")
    torch.cuda.synchronize()
    assert (call.logp2 == SENT).all() and not (call.dl[:, :, :V] == SENT).any()
    call.fresh()
    saved = call.set.in_xg
    call.set.in_xg = None
    rejected(call.score, call.score_args(), "null table")
    call.set.in_xg = saved
    a = call.grad_args()
    a.normalized = 1
    rejected(call.grad, a, "normalized")
    a = call.grad_args()
    a.dlogits = a.logits
    rejected(call.grad, a, "alias")
    for fn, mk in ((call.score, call.score_args), (call.grad, call.grad_args)):
        a = mk()
        a.ldv = V - 1
        rejected(fn, a, "ldv")
        a = mk()
        a.V = 2                                                             # U = 2 >= V
        rejected(fn, a, "U=")
        for T_bad in (0, (1 << 20) + 1):
            a = mk()
            a.T = T_bad
            rejected(fn, a, "bad shape")
        a = mk()
        a.workspace = a.workspace + 4
        rejected(fn, a, "aligned")
    with pytest.raises(ValueError):
        ops.ctc_graph_logp(call.buf[:, :, :3].contiguous(), call.hl, DecodingGraph.token_loop(4))       # U = V
    with pytest.raises(TypeError):
        ops.ctc_graph_logp(call.buf, call.hl, [[1, 2]])


# ---------------------------------------------------------------- 12: ops and the model ----
def test_ops_autograd_against_the_restatement():
    rng = np.random.default_rng(121)
    B, T, V = 3, 19, 10
    graphs = [DecodingGraph.from_alternatives([[[1], [2, 3]], [[4], []], [[5]], [[1, 1], [6]]], [[0.0, -0.5], [-0.1, -1.0], [0.0], [0.0, 0.2]]),
              R.random_graph(rng, 7, 22, V, final_p=0.6)]
    graph_of = [1, 0, 0]
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    hlens, w = np.array([T, 14, T], dtype=np.int32), np.array([1.0, -0.5, 3.0], dtype=np.float32)
    want_lp, want_dl = R.logp_and_grad(logits, hlens, graphs, graph_of, g=w.astype(np.float64))
    # a [..., :V] view of padded rows is taken as it is
    padded = torch.zeros(B, T, 12, device=DEV)
    padded[..., :V] = torch.from_numpy(logits).to(DEV)
    for x in (torch.from_numpy(logits).to(DEV).requires_grad_(True), padded.requires_grad_(True)):
        view = x if x.shape[-1] == V else x[..., :V]
        out = ops.ctc_graph_logp(view, torch.from_numpy(hlens).to(DEV), graphs, torch.tensor(graph_of, device=DEV))
        (torch.from_numpy(w).to(DEV) * out).sum().backward()
        check_logp(out.detach().cpu().numpy(), want_lp, "ops")
        check_grad(x.grad[..., :V].cpu().numpy(), want_dl, w, "ops autograd")
        assert not x.grad[..., V:].any()


def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), {k: v.to(DEV) for k, v in g["in"].items()}


def test_model_graph_loss_and_posterior():
    model, i = tiny_conformer()
    feats, flen, tgt, tlen = i["feats"], i["flen"], i["tgt"], i["tlen"]
    B = feats.shape[0]
    graphs = [DecodingGraph.linear(tgt[b, :int(tlen[b])].tolist()) for b in range(B)]
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        lens = mask.squeeze(1).sum(1)
        plain = float(model.ctc(enc, lens, tgt, tlen))
    model.ctc_weight, keep = 1.0, model.ctc_weight
    loss, info = model.ctc_graph_loss(feats, flen, graphs, graph_of=torch.arange(B, device=DEV))
    model.ctc_weight = keep
    assert info["acc"] is None and bool(info["feasible"].all()) and info["logp"].shape == (B,)
    check_logp([float(loss.detach()) * B], [plain * B], "model: graph loss of linear chains vs the CTC head")
    loss.backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert model.ctc.ctc_lo.weight.grad is not None and float(model.ctc.ctc_lo.weight.grad.abs().sum()) > 0
    joint, info2 = model.ctc_graph_loss(feats, flen, graphs, torch.arange(B, device=DEV), targets=tgt, targets_length=tlen)
    assert info2["acc"] is not None and np.isfinite(float(joint)) and np.array_equal(bits(info2["logp"]), bits(info["logp"]))
    # the rejection score of ctc_graph_search
    gr = DecodingGraph.from_phrases([graphs[0].label.tolist(), graphs[1].label.tolist(), [1, 2, 3]])
    before = model.ctc_graph_search(feats, flen, gr)
    with_post = model.ctc_graph_search(feats, flen, gr, posterior=True)
    with torch.no_grad():
        logits, lens = model.ctc_logits_windowed(feats, flen, None, 16)
        mass = ops.ctc_graph_logp(logits, lens, gr).cpu().tolist()
    for a, b, m in zip(before, with_post, mass):
        assert a.log_mass is None and a.posterior is None
        assert (a.feasible, a.score, a.tokens, a.traversals, a.outputs) == (b.feasible, b.score, b.tokens, b.traversals, b.outputs)
        assert b.feasible and b.log_mass == m and 0.0 < b.posterior <= 1.0
        assert b.score <= m + ATOL
