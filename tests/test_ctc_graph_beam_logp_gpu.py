"""GPU: the beam-pruned graph CTC likelihood and its gradient (oe_ctc_graph_beam_logp / oe_ctc_graph_beam_logp_grad) through the
C ABI against the float64 restatement (ctc_graph_beam_logp_ref.py), and through ops.ctc_graph_beam_logp,
ASRModel.ctc_graph_search(posterior_beam=...) and ASRModel.ctc_graph_loss(denominator=...).

Tolerances: oe_ctc_graph_logp's - logp rtol 1e-4 / atol 1e-3, gradient rtol 2e-3 / atol 2e-5 * |g[b]| - against the float64
restatement, never against the code under test.  Every comparison prints the worst fraction of its tolerance it used (`-s`
shows them; DESIGN.md records the measured ones).

Pruning makes the comparison discrete: a state within rounding of a threshold may flip.  So every comparison first asserts, from
the restatement alone, one of
  (a) guard band: gap >= 0.02 - the survivor sets are then identical, and status and peak are compared exactly;
  (b) sensitivity: the restatement at beam - 1e-3 and beam + 1e-3 differs from that at beam by at most a tenth of the tolerance.
Where a test claims that pruning matters it also asserts that the restatement at the beam differs from the unpruned one by more
than the tolerance.

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_graph_beam_logp_ref as P  # noqa: E402
import ctc_graph_logp_ref as R  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.utils.decoding_graph import (BEAM_MAX_ARCS, BEAM_MAX_NODES, LOGP_MAX_ARCS, LOGP_MAX_NODES, DecodingGraph,  # noqa: E402
                                              GraphSet)

DEV = "cuda"
INF = float("inf")
RTOL, ATOL = 1e-4, 1e-3
G_RTOL, G_ATOL = 2e-3, 2e-5
SENT, ISENT = 5.0, -77
OK, INFEASIBLE, OVERFLOW = 0, 1, 2


class Call:
    """oe_ctc_graph_beam_logp and oe_ctc_graph_beam_logp_grad on one batch, sentinel-filled outputs; the columns behind V hold 3.0."""

    def __init__(self, logits, hlens, graph, beam, max_active=None, g=None, normalized=False, ldv=None):
        logits = torch.as_tensor(np.asarray(logits), dtype=torch.float32)
        self.B, self.T, self.V = (int(s) for s in logits.shape)
        self.ldv = ldv or self.V
        self.buf = torch.full((self.B, self.T, self.ldv), 3.0, device=DEV)
        self.buf[:, :, :self.V] = logits.to(DEV)
        self.graph, self.gr = graph, hip.beam_logp_graph(graph, DEV)
        self.hl = torch.as_tensor(np.asarray(hlens), dtype=torch.int32).to(DEV)
        self.g = torch.as_tensor(np.ones(self.B) if g is None else np.asarray(g), dtype=torch.float32).to(DEV)
        self.normalized, self.beam = int(normalized), float(beam)
        self.max_active = graph.num_nodes + graph.num_arcs if max_active is None else int(max_active)
        lib = hip.lib()
        shape = (self.B, self.T, len(graph.cols), graph.num_nodes, graph.num_arcs, self.max_active)
        self.ws = torch.empty(max(lib.oe_ctc_graph_beam_logp_workspace_bytes(*shape), 16), dtype=torch.uint8, device=DEV)
        self.gws = torch.empty(max(lib.oe_ctc_graph_beam_logp_grad_workspace_bytes(*shape), 16), dtype=torch.uint8, device=DEV)
        self.fresh()

    def fresh(self):
        f = lambda: torch.full((self.B,), SENT, device=DEV)
        i = lambda: torch.full((self.B,), ISENT, dtype=torch.int32, device=DEV)
        self.logp, self.logp2, self.status, self.peak, self.status2, self.peak2 = f(), f(), i(), i(), i(), i()
        self.dl = torch.full((self.B, self.T, self.ldv), SENT, device=DEV)

    def _common(self, a, ws):
        a.logits, a.ldv, a.B, a.T, a.V = self.buf.data_ptr(), self.ldv, self.B, self.T, self.V
        a.hlens, a.graph, a.workspace = self.hl.data_ptr(), C.pointer(self.gr), ws.data_ptr()
        a.normalized, a.max_active, a.beam = self.normalized, self.max_active, self.beam
        return a

    def score_args(self):
        a = self._common(hip.CtcGraphBeamLogpArgs(), self.ws)
        a.logp, a.status, a.peak = self.logp.data_ptr(), self.status.data_ptr(), self.peak.data_ptr()
        return a

    def grad_args(self):
        a = self._common(hip.CtcGraphBeamLogpGradArgs(), self.gws)
        a.g, a.dlogits, a.logp = self.g.data_ptr(), self.dl.data_ptr(), self.logp2.data_ptr()
        a.status, a.peak = self.status2.data_ptr(), self.peak2.data_ptr()
        return a

    def score(self, a=None):
        return hip.lib().oe_ctc_graph_beam_logp(C.byref(a or self.score_args()), hip.stream())

    def grad(self, a=None):
        return hip.lib().oe_ctc_graph_beam_logp_grad(C.byref(a or self.grad_args()), hip.stream())

    def run(self, grad=True):
        hip.check(self.score(), "oe_ctc_graph_beam_logp")
        if grad:
            hip.check(self.grad(), "oe_ctc_graph_beam_logp_grad")
        torch.cuda.synchronize()
        if grad:                                                             # the two entries agree in every bit
            assert np.array_equal(bits(self.logp), bits(self.logp2))
            assert torch.equal(self.status, self.status2) and torch.equal(self.peak, self.peak2)
            assert bool((self.dl[:, :, self.V:] == SENT).all())              # the columns behind V are never written
        return self

    def outputs(self):
        return self.logp, self.logp2, self.status, self.peak, self.status2, self.peak2, self.dl

    def untouched(self):
        return all(bool((t == (ISENT if t.dtype == torch.int32 else SENT)).all()) for t in self.outputs())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def logp_fraction(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf]), (got, want)                  # -inf exactly
    frac = np.abs(got[~inf] - want[~inf]) / (ATOL + RTOL * np.abs(want[~inf]))
    return float(frac.max()) if frac.size else 0.0


def check_logp(got, want, what):
    worst = logp_fraction(got, want)
    print(f"FRACTION logp {what}: {worst:.4f}")
    assert worst <= 1.0, (what, got, want)
    return worst


def grad_fraction(got, want, g):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = G_ATOL * np.abs(np.asarray(g, dtype=np.float64))[:, None, None] + G_RTOL * np.abs(want)
    tol = np.where(np.isfinite(tol), tol, 0.0)                              # g = NaN: an infeasible utterance, exact zeros
    err = np.abs(got - want)
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))))


def check_grad(got, want, g, what):
    worst = grad_fraction(got, want, g)
    print(f"FRACTION grad {what}: {worst:.4f}")
    assert worst <= 1.0, what
    return worst


def restate(logits, hlens, graph, beam, g, fast=False):
    return P.logp_and_grad(logits, hlens, graph, beam, g=np.nan_to_num(np.asarray(g, dtype=np.float64)), fast=fast)


def status_of(results):
    return [OK if np.isfinite(r["logz"]) else INFEASIBLE for r in results]


def peak_of(results):
    return [max(r["survivors"], default=0) for r in results]


def assert_insensitive(logits, hlens, graph, beam, g, want, grad, fast=False):
    """Condition (b): the restatement at beam -+ 1e-3 within a tenth of the tolerance of the one at beam."""
    for d in (-1e-3, 1e-3):
        lp, dl, _ = restate(logits, hlens, graph, beam + d, g, fast)
        assert logp_fraction(lp, want[0]) <= 0.1, (beam, d)
        if grad:
            assert grad_fraction(dl, want[1], g) <= 0.1, (beam, d)


def recipe(seed, Q, A, V, T):
    rng = np.random.default_rng(seed)
    g = R.random_graph(rng, Q, A, V)
    return g, (rng.normal(size=(1, T, V)) * 2.0)


# ---------------------------------------------------------------- the three shapes ----
@pytest.mark.parametrize("seed", [1, 6, 7, 8])
def test_guard_banded_small_shape(seed):
    """(a): every state is 0.02 away from its threshold, so the survivor sets, status and peak are exact."""
    Q, A, V, T, beam = 12, 40, 9, 12, 4.0
    graph, logits = recipe(seed, Q, A, V, T)
    g = np.array([1.5], dtype=np.float32)
    want = restate(logits, [T], graph, beam, g)
    assert want[2][0]["gap"] >= 0.02 and want[2][0]["cut"] >= 100
    call = Call(logits, [T], graph, beam, g=g, ldv=V + 3).run()
    assert call.status.tolist() == status_of(want[2]) and call.peak.tolist() == peak_of(want[2])
    check_logp(call.logp.cpu().numpy(), want[0], f"guard band seed {seed}")
    check_grad(call.dl[:, :, :V].cpu().numpy(), want[1], g, f"guard band seed {seed}")
    full = restate(logits, [T], graph, INF, g)
    assert logp_fraction(full[0], want[0]) > 1.0                             # pruning matters: the unpruned sum is another number


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_40_nodes(seed):
    """(b) for logp and the gradient: no state sits within 1e-3 of a threshold."""
    Q, A, V, T, beam = 40, 200, 20, 16, 12.0
    graph, logits = recipe(seed, Q, A, V, T)
    g = np.array([-2.0], dtype=np.float32)
    want = restate(logits, [T], graph, beam, g)
    assert_insensitive(logits, [T], graph, beam, g, want, grad=True)
    assert want[2][0]["cut"] >= 200
    call = Call(logits, [T], graph, beam, g=g).run()
    assert call.status.tolist() == [OK]
    check_logp(call.logp.cpu().numpy(), want[0], f"40 nodes seed {seed}")
    check_grad(call.dl.cpu().numpy(), want[1], g, f"40 nodes seed {seed}")
    assert grad_fraction(restate(logits, [T], graph, INF, g)[1], want[1], g) > 1.0     # pruning matters for the occupancies


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_300_nodes(seed):
    """(b): at beam 12 for logp only (thousands of states are cut, some within 1e-3 of a threshold), at beam 16 for the gradient."""
    Q, A, V, T = 300, 1500, 50, 24
    graph, logits = recipe(seed, Q, A, V, T)
    g = np.array([1.0], dtype=np.float32)
    want = restate(logits, [T], graph, 12.0, g)
    assert_insensitive(logits, [T], graph, 12.0, g, want, grad=False)
    assert want[2][0]["cut"] >= 5000
    call = Call(logits, [T], graph, 12.0, g=g).run()
    assert call.status.tolist() == [OK]
    check_logp(call.logp.cpu().numpy(), want[0], f"300 nodes beam 12 seed {seed}")
    want = restate(logits, [T], graph, 16.0, g)
    assert_insensitive(logits, [T], graph, 16.0, g, want, grad=True)
    call = Call(logits, [T], graph, 16.0, g=g).run()
    check_logp(call.logp.cpu().numpy(), want[0], f"300 nodes beam 16 seed {seed}")
    check_grad(call.dl.cpu().numpy(), want[1], g, f"300 nodes beam 16 seed {seed}")


# ---------------------------------------------------------------- beam = inf: the dense kernel's problem ----
def unpruned(graph, logits, hlens, g, what, fast=True, restatement=True):
    """beam = inf against the restatement and against oe_ctc_graph_logp on the device."""
    call = Call(logits, hlens, graph, INF, g=g).run()
    assert call.status.tolist() == [OK if np.isfinite(x) else INFEASIBLE for x in call.logp.tolist()]
    if restatement:
        want = restate(logits, hlens, graph, INF, g, fast)
        check_logp(call.logp.cpu().numpy(), want[0], what)
        check_grad(call.dl.cpu().numpy(), want[1], g, what)
    x = torch.as_tensor(np.asarray(logits), dtype=torch.float32).to(DEV).requires_grad_(True)
    dense = ops.ctc_graph_logp(x, call.hl, graph)
    finite = torch.isfinite(dense.detach())
    (call.g * torch.where(finite, dense, torch.zeros_like(dense))).sum().backward()
    check_logp(call.logp.cpu().numpy(), dense.detach().double().cpu().numpy(), what + " vs oe_ctc_graph_logp")
    check_grad(call.dl.cpu().numpy(), x.grad.double().cpu().numpy(), g, what + " vs oe_ctc_graph_logp_grad")
    return call


def test_unpruned_random_graph():
    rng = np.random.default_rng(21)
    V, T = 9, 23
    graph = R.random_graph(rng, 11, 38, V, final_p=0.5)
    logits = (rng.normal(size=(3, T, V)) * 2.0).astype(np.float32)
    unpruned(graph, logits, [T, 17, 9], np.array([1.0, -0.5, 2.5], dtype=np.float32), "unpruned random graph", fast=False)


def test_unpruned_token_loop():
    """One node, 299 leaving arcs (a wave's), 299 in-groups of one arc: with raw logits logZ = 0 and the gradient is zero."""
    rng = np.random.default_rng(300)
    V, T = 300, 19
    logits = (rng.normal(size=(2, T, V)) * 3.0).astype(np.float32)
    logits[1, :, 5] += 12.0
    g = np.array([1.5, -2.0], dtype=np.float32)
    call = unpruned(DecodingGraph.token_loop(V), logits, [T, T - 3], g, "token loop V=300", restatement=False)
    logp, dl = call.logp.cpu().numpy(), call.dl.cpu().numpy()
    print(f"FRACTION logp token loop: {np.abs(logp).max() / ATOL:.4f}")
    print(f"FRACTION grad token loop: {(np.abs(dl) / (G_ATOL * np.abs(g))[:, None, None]).max():.4f}")
    assert (np.abs(logp) <= ATOL).all() and (np.abs(dl) <= (G_ATOL * np.abs(g))[:, None, None]).all()


def looped_trie(rng, V, n):
    phrases = set()
    while len(phrases) < n:
        k = int(rng.integers(1, 5))
        phrases.add(tuple(int(x) for x in rng.integers(1, V, size=k - 1)) + (int(rng.choice([3, 3, 7, 7, int(rng.integers(1, V))])),))
    phrases = sorted(phrases)
    return phrases, [-0.1 * (i % 7) for i in range(len(phrases))]


def test_unpruned_looped_trie():
    rng = np.random.default_rng(41)
    V, T = 14, 40
    phrases, weights = looped_trie(rng, V, 50)
    graph = DecodingGraph.from_phrases(phrases, weights=weights, loop=True)
    in_grp, in_xg, _, out_xg, _ = graph.host_group_tables()
    assert np.bincount(in_grp).max() > 1 and (in_xg >= 0).any() and (out_xg >= 0).any()     # groups of several arcs; arcs matching a group
    logits = (rng.normal(size=(2, T, V)) * 1.5).astype(np.float32)
    unpruned(graph, logits, [T, 33], np.array([1.0, -1.25], dtype=np.float32), "looped trie")


def wide_dag(rng, Q, A, V):
    arcs = [(0, 1, 1, 0.0), (int(rng.integers(0, 2)), 2, 2, 0.0)]
    arcs += [(int(rng.integers(0, 3)), q, int(rng.integers(1, V)), float(rng.normal() * 0.3)) for q in range(3, Q)]
    arcs += [(int(rng.integers(0, 40)), Q - 1, int(rng.integers(1, 6)), 0.0) for _ in range(40)]
    while len(arcs) < A:
        s = int(rng.integers(0, Q - 1))
        arcs.append((s, int(rng.integers(s + 1, Q)), int(rng.integers(1, V)), float(rng.normal() * 0.3)))
    return DecodingGraph(Q, arcs, {int(q): 0.0 for q in rng.choice(Q, size=Q // 3, replace=False)})


def test_unpruned_at_the_dense_limits():
    rng = np.random.default_rng(61)
    V, T = 50, 4
    graph = wide_dag(rng, LOGP_MAX_NODES, LOGP_MAX_ARCS, V)
    assert (graph.num_nodes, graph.num_arcs) == (LOGP_MAX_NODES, LOGP_MAX_ARCS)
    logits = (rng.normal(size=(2, T, V)) * 2.0).astype(np.float32)
    unpruned(graph, logits, [T, 3], np.array([1.0, 2.0], dtype=np.float32), "at the dense limits")


def test_unpruned_nodes_of_many_leaving_arcs():
    """A node of 20 leaving arcs (above 16: a wave takes it) and one of 70 (more than one round of the wave)."""
    rng = np.random.default_rng(71)
    V, T = 12, 14
    arcs = [(0, 1 + i, 1 + i % (V - 1), float(rng.normal() * 0.3)) for i in range(20)]
    arcs += [(1, 21 + i, 1 + i % (V - 1), float(rng.normal() * 0.3)) for i in range(70)]
    arcs += [(int(rng.integers(2, 91)), int(rng.integers(0, 91)), int(rng.integers(1, V)), float(rng.normal() * 0.3)) for _ in range(120)]
    graph = DecodingGraph(91, arcs, {int(q): 0.0 for q in rng.choice(91, size=30, replace=False)})
    deg = np.diff(graph.out_ptr)
    assert deg[0] > 16 and deg[1] > 64
    logits = (rng.normal(size=(2, T, V)) * 2.0).astype(np.float32)
    unpruned(graph, logits, [T, 9], np.array([1.0, -3.0], dtype=np.float32), "wide nodes", fast=False)


# ---------------------------------------------------------------- beyond the dense limits ----
def big_lexicon(n_words=5000, V=40, seed=5, extra=()):
    rng = np.random.default_rng(seed)
    words = set(extra)
    while len(words) < n_words:
        words.add(tuple(int(x) for x in rng.integers(1, V, size=int(rng.integers(2, 6)))))
    words = sorted(words)
    return DecodingGraph.from_phrases(words, weights=[-0.05 * (i % 9) for i in range(len(words))], loop=True, large=True)


def test_large_lexicon_loop():
    """About 5000 words: more nodes and arcs than oe_ctc_graph_logp holds.  Against the fast restatement under (b): at beam 10
    for logp (57000 states are cut, the nearest 7e-6 from its threshold; the restatement moves by 0.03 of the logp tolerance
    over beam -+ 1e-3 but by 0.9 of the gradient's), at beam 14 for the gradient (0.02 of its tolerance)."""
    graph = big_lexicon()
    assert graph.num_nodes > LOGP_MAX_NODES and graph.num_arcs > LOGP_MAX_ARCS
    with pytest.raises(ValueError):
        GraphSet([graph])
    rng = np.random.default_rng(9)
    V, T = 40, 16
    logits = (rng.normal(size=(2, T, V)) * 2.0).astype(np.float32)
    hlens, g = [T, 11], np.array([1.0, -0.75], dtype=np.float32)
    full = restate(logits, hlens, graph, INF, g, fast=True)
    for beam, grad in ((10.0, False), (14.0, True)):
        want = restate(logits, hlens, graph, beam, g, fast=True)
        assert np.isfinite(want[0]).all() and all(r["cut"] > 30000 for r in want[2])
        assert_insensitive(logits, hlens, graph, beam, g, want, grad=grad, fast=True)
        assert (grad_fraction(full[1], want[1], g) if grad else logp_fraction(full[0], want[0])) > 1.0        # pruning matters
        call = Call(logits, hlens, graph, beam, max_active=16384, g=g).run()
        print(f"large lexicon beam {beam}:", graph.num_nodes, "nodes", graph.num_arcs, "arcs; peak", call.peak.tolist(), "restated",
              peak_of(want[2]))
        assert call.status.tolist() == [OK, OK]
        check_logp(call.logp.cpu().numpy(), want[0], f"large lexicon loop beam {beam}")
        if grad:
            check_grad(call.dl.cpu().numpy(), want[1], g, f"large lexicon loop beam {beam}")


# ---------------------------------------------------------------- edge cases ----
def test_lengths_infeasible_and_nan_g():
    rng = np.random.default_rng(81)
    V, T = 9, 12
    graph = R.random_graph(rng, 10, 36, V, final_p=0.5)
    logits = (rng.normal(size=(4, T, V)) * 2.0).astype(np.float32)
    hlens = [0, 1, 7, T]
    g = np.array([np.nan, 1.0, -0.5, 2.0], dtype=np.float32)
    call = Call(logits, hlens, graph, INF, g=g, ldv=V + 1).run()
    want = restate(logits, hlens, graph, INF, g)
    assert call.status.tolist() == status_of(want[2]) and call.status[0].item() == INFEASIBLE
    assert call.peak.tolist() == peak_of(want[2]) and call.peak[0].item() == 0
    check_logp(call.logp.cpu().numpy(), want[0], "lengths 0, 1, < T")
    check_grad(call.dl[:, :, :V].cpu().numpy(), want[1], g, "lengths 0, 1, < T")
    assert call.logp[0].item() == -INF and not call.dl[0, :, :V].any()       # NaN g is not read into a result
    assert not call.dl[2, 7:, :V].any()                                       # rows t >= Tb are exact zeros
    # infeasible by construction: the final node is unreachable
    dead = DecodingGraph(4, [(0, 1, 2, 0.0), (1, 1, 3, -0.5), (2, 3, 1, 0.0)], {3: 0.0})
    call = Call(logits[:2], [T, 5], dead, INF, g=np.array([np.nan, np.nan], dtype=np.float32)).run()
    assert call.status.tolist() == [INFEASIBLE] * 2 and call.logp.tolist() == [-INF] * 2 and not call.dl.any()


def test_infeasible_by_pruning_alone():
    """Label 1 leads into a dead end and dominates frame 0; the accepted path (label 2) is cut there by a narrow beam."""
    graph = DecodingGraph(3, [(0, 1, 1, 0.0), (0, 2, 2, 0.0)], {2: 0.0})
    T, V = 4, 3
    lp = np.log(np.tile(np.array([0.02, 0.9, 0.08]), (1, T, 1)))
    g = np.array([np.nan], dtype=np.float32)
    narrow, wide = P.pruned_logp(lp[0], graph, 1.0), P.pruned_logp(lp[0], graph, INF)
    assert narrow["logz"] == -np.inf and narrow["gap"] >= 0.02 and np.isfinite(wide["logz"])
    call = Call(lp, [T], graph, 1.0, g=g, normalized=True).run(grad=False)
    assert call.status.tolist() == [INFEASIBLE] and call.logp.tolist() == [-INF] and call.peak.tolist() == [max(narrow["survivors"])]
    call = Call(np.log(np.exp(lp)), [T], graph, 1.0, g=g).run()                  # raw logits that are already normalised
    assert call.status.tolist() == [INFEASIBLE] and call.logp.tolist() == [-INF] and not call.dl.any()
    call = Call(lp, [T], graph, INF, normalized=True).run(grad=False)
    check_logp(call.logp.cpu().numpy(), [wide["logz"]], "the same utterance without a beam")


def test_overflow_reports_the_first_overflowing_count():
    rng = np.random.default_rng(91)
    V, T = 9, 12
    graph = R.random_graph(rng, 10, 36, V, final_p=0.5)
    logits = (rng.normal(size=(2, T, V)) * 2.0).astype(np.float32)
    hlens = [T, 2]
    want = restate(logits, hlens, graph, INF, [1.0, 1.0])
    surv = [r["survivors"] for r in want[2]]
    cap = max(surv[1])                                                        # the short utterance fits, the long one does not
    assert max(surv[0]) > cap
    call = Call(logits, hlens, graph, INF, max_active=cap, g=np.array([np.nan, 1.0], dtype=np.float32)).run()
    assert call.status.tolist() == [OVERFLOW, OK]
    assert call.peak.tolist() == [next(n for n in surv[0] if n > cap), cap]
    assert call.logp[0].item() == -INF and not call.dl[0].any()
    check_logp(call.logp[1:].cpu().numpy(), want[0][1:], "beside an overflowed utterance")
    check_grad(call.dl[1:].cpu().numpy(), want[1][1:], [1.0], "beside an overflowed utterance")


def test_runs_are_bit_equal_and_utterances_independent():
    graph, _ = recipe(2, 40, 200, 20, 16)
    rng = np.random.default_rng(5)
    B, T, V = 5, 16, 20
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    hlens = np.array([T, 9, T, 13, 4], dtype=np.int32)
    g = np.array([1.0, -1.0, 0.5, 2.0, 3.0], dtype=np.float32)
    a, b = Call(logits, hlens, graph, 8.0, g=g).run(), Call(logits, hlens, graph, 8.0, g=g).run()
    for x, y in zip(a.outputs(), b.outputs()):
        assert np.array_equal(bits(x), bits(y))
    perm = np.array([3, 0, 4, 2, 1])
    c = Call(logits[perm], hlens[perm], graph, 8.0, g=g[perm]).run()
    for x, y in zip(a.outputs(), c.outputs()):
        assert np.array_equal(bits(x)[perm], bits(y))
    assert a.status.tolist() == [OK] * B


# ---------------------------------------------------------------- arguments ----
def test_bad_arguments_are_reported_not_launched():
    rng = np.random.default_rng(3)
    V, T = 9, 6
    graph = R.random_graph(rng, 6, 20, V)
    call = Call(rng.normal(size=(2, T, V)), [T, 4], graph, 4.0)
    lib = hip.lib()

    def rejected(entry, args, change):
        call.fresh()
        a = args()
        if change is not None:
            change(a)
        assert entry(a) != 0 and lib.oe_last_error()
        torch.cuda.synchronize()
        assert call.untouched(), lib.oe_last_error()

    def setter(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a, k, v)
        return f

    shared = [setter(logits=None), setter(hlens=None), setter(workspace=None), setter(status=None), setter(peak=None),
              setter(B=0), setter(T=0), setter(T=(1 << 20) + 1), setter(V=1), setter(ldv=V - 1), setter(max_active=0),
              setter(beam=-1.0), setter(beam=float("nan"))]
    for entry, args in ((call.score, call.score_args), (call.grad, call.grad_args)):
        for s in shared:
            rejected(entry, args, s)
        rejected(entry, args, lambda a: setattr(a, "workspace", a.workspace + 8))       # not 16-byte aligned
    rejected(call.score, call.score_args, setter(logp=None))
    for s in (setter(g=None), setter(dlogits=None), setter(normalized=1), setter(dlogits=call.buf.data_ptr())):
        rejected(call.grad, call.grad_args, s)
    null_graph = setter(graph=C.POINTER(hip.BeamLogpGraph)())
    rejected(call.score, call.score_args, null_graph)
    rejected(call.grad, call.grad_args, null_graph)
    for field in ("in_ptr", "src", "dst", "label", "col", "w", "final", "cols", "out_ptr", "out_arc", "in_grp", "in_xg", "out_grp", "out_xg",
                  "inv"):
        keep = getattr(call.gr, field)
        setattr(call.gr, field, None)
        rejected(call.score, call.score_args, None)
        rejected(call.grad, call.grad_args, None)
        setattr(call.gr, field, keep)
    for field, bad in (("Q", 0), ("Q", BEAM_MAX_NODES + 1), ("A", 0), ("A", BEAM_MAX_ARCS + 1), ("U", 0), ("U", V), ("n_inv", -1)):
        keep = getattr(call.gr, field)
        setattr(call.gr, field, bad)
        rejected(call.score, call.score_args, None)
        rejected(call.grad, call.grad_args, None)
        setattr(call.gr, field, keep)
    call.fresh()
    call.run()                                                                # and the call still works
    assert not (call.logp == SENT).any() and not (call.dl[:, :, :V] == SENT).any()


def test_size_functions_return_zero_outside_the_limits():
    lib = hip.lib()
    for fn in (lib.oe_ctc_graph_beam_logp_workspace_bytes, lib.oe_ctc_graph_beam_logp_grad_workspace_bytes):
        assert fn(2, 8, 5, BEAM_MAX_NODES, BEAM_MAX_ARCS, 64) > 0
        assert fn(2, 8, 5, BEAM_MAX_NODES + 1, 8, 64) == 0 and fn(2, 8, 5, 8, BEAM_MAX_ARCS + 1, 64) == 0
        assert fn(0, 8, 5, 8, 8, 64) == 0 and fn(2, 0, 5, 8, 8, 64) == 0 and fn(2, (1 << 20) + 1, 5, 8, 8, 64) == 0
        assert fn(2, 8, 0, 8, 8, 64) == 0 and fn(2, 8, 5, 0, 8, 64) == 0 and fn(2, 8, 5, 8, 0, 64) == 0 and fn(2, 8, 5, 8, 8, 0) == 0
    # the formulas of include/openeat_hip.h
    B, T, U, Q, A, M = 3, 10, 5, 9, 22, 17
    up4, up16 = lambda n: (n + 3) & ~3, lambda n: (n + 15) & ~15
    rows = up16(4 * B * T * (U + 1))
    assert lib.oe_ctc_graph_beam_logp_workspace_bytes(B, T, U, Q, A, M) == rows + B * (52 * up4(Q) + 24 * up4(A) + 60 * up4(M))
    assert lib.oe_ctc_graph_beam_logp_grad_workspace_bytes(B, T, U, Q, A, M) == 3 * rows + up16(4 * B * T) + up16(8 * B) + B * (
        64 * up4(Q) + 36 * up4(A) + 60 * up4(M) + 4 * up4(T) + 12 * T * up4(M))
    assert lib.oe_ctc_graph_beam_logp_workspace_bytes(B, T, U, Q, A, 1000) == lib.oe_ctc_graph_beam_logp_workspace_bytes(B, T, U, Q, A, Q + A)


# ---------------------------------------------------------------- ops and the model ----
def test_ops_autograd_and_utterance_groups():
    Q, A, V, T, beam = 40, 200, 20, 16, 12.0
    graph, _ = recipe(1, Q, A, V, T)
    rng = np.random.default_rng(17)
    B = 3
    logits = (rng.normal(size=(B, T, V)) * 2.0).astype(np.float32)
    hlens, w = np.array([T, 11, T], dtype=np.int32), np.array([1.0, -0.5, 3.0], dtype=np.float32)
    want = restate(logits, hlens, graph, beam, w)
    assert_insensitive(logits, hlens, graph, beam, w, want, grad=True)
    padded = torch.zeros(B, T, V + 4, device=DEV)
    padded[..., :V] = torch.from_numpy(logits).to(DEV)
    hl, wt = torch.from_numpy(hlens).to(DEV), torch.from_numpy(w).to(DEV)
    kept = []
    lib = hip.lib()
    tight = lib.oe_ctc_graph_beam_logp_grad_workspace_bytes(1, T, len(graph.cols), Q, A, 16384)
    for x, cap in ((torch.from_numpy(logits).to(DEV).requires_grad_(True), 1 << 30), (padded.requires_grad_(True), 1 << 30),
                   (torch.from_numpy(logits).to(DEV).requires_grad_(True), tight)):          # three groups of one, both directions
        view = x if x.shape[-1] == V else x[..., :V]
        logp, status, peak = ops.ctc_graph_beam_logp(view, hl, graph, beam, workspace_cap=cap)
        assert not status.requires_grad and status.tolist() == [OK] * B and peak.dtype == torch.int32
        (wt * logp).sum().backward()
        check_logp(logp.detach().cpu().numpy(), want[0], "ops")
        check_grad(x.grad[..., :V].cpu().numpy(), want[1], w, "ops autograd")
        assert not x.grad[..., V:].any()
        kept.append((logp.detach(), x.grad[..., :V].contiguous()))
    for lp, gr in kept[1:]:                                                  # padded rows and utterance groups: the bits of one call
        assert np.array_equal(bits(lp), bits(kept[0][0])) and np.array_equal(bits(gr), bits(kept[0][1]))
    with pytest.raises(TypeError):
        ops.ctc_graph_beam_logp(kept[0][1], hl, [[1, 2]], beam)
    for bad in (dict(beam=-1.0), dict(beam=float("nan")), dict(beam=2.0, max_active=0)):
        with pytest.raises(ValueError):
            ops.ctc_graph_beam_logp(kept[0][1], hl, graph, **bad)
    with pytest.raises(ValueError):
        ops.ctc_graph_beam_logp(kept[0][1].requires_grad_(True), hl, graph, beam, normalized=True)


def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), {k: v.to(DEV) for k, v in g["in"].items()}


def test_model_posterior_beam_and_denominator(monkeypatch):
    model, i = tiny_conformer()
    feats, flen, tgt, tlen = i["feats"], i["flen"], i["tgt"], i["tlen"]
    B, V = feats.shape[0], model.vocab_size
    big = big_lexicon(5000, V - 1, 4, extra={tuple(tgt[b, :int(tlen[b])].tolist()) for b in range(B)})
    assert big.num_nodes > LOGP_MAX_NODES and big.num_arcs > LOGP_MAX_ARCS
    with pytest.raises(ValueError, match="posterior"):
        model.ctc_graph_search(feats, flen, big, beam=8.0, posterior=True)      # alone it still raises
    res = model.ctc_graph_search(feats, flen, big, beam=8.0, posterior_beam=12.0)
    with torch.no_grad():
        logits, lens = model.ctc_logits_windowed(feats, flen, None, 16)
        mass, status, _ = ops.ctc_graph_beam_logp(logits, lens, big, 12.0)
    assert status.tolist() == [OK] * B
    for r, m in zip(res, mass.cpu().tolist()):
        assert r.feasible and r.log_mass == m and np.isfinite(m) and 0.0 < r.posterior <= 1.0
    # an overflowing capacity is doubled until it fits, and the result is the same
    asked = []
    real = ops.ctc_graph_beam_logp
    monkeypatch.setattr(ops, "ctc_graph_beam_logp", lambda *a, **k: asked.append((a[0].shape[0], a[4])) or real(*a, **k))
    small = model.ctc_graph_search(feats, flen, big, beam=8.0, max_active=64, posterior_beam=12.0)
    assert [r.log_mass for r in small] == [r.log_mass for r in res] and len(asked) >= 2 and asked[0] == (B, 64)
    monkeypatch.undo()
    # the MMI-style loss: numerator the transcripts' chains, denominator the lexicon loop
    graphs = [DecodingGraph.linear(tgt[b, :int(tlen[b])].tolist()) for b in range(B)]
    graph_of = torch.arange(B, device=DEV)
    model.ctc_weight, keep = 1.0, model.ctc_weight
    model.zero_grad()
    loss, info = model.ctc_graph_loss(feats, flen, graphs, graph_of, denominator=big, den_beam=12.0, den_scale=0.5)
    assert bool(info["feasible"].all()) and info["logp_den"].shape == (B,)
    want_loss = -(info["logp"].double() - 0.5 * info["logp_den"].double()).sum() / B
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-4 * max(1.0, abs(float(want_loss)))
    loss.backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert model.ctc.ctc_lo.weight.grad is not None and float(model.ctc.ctc_lo.weight.grad.abs().sum()) > 0
    model.ctc_weight = keep
    # the loss's gradient with respect to the CTC logits against the two restatements combined
    got, lg, lens = dlogits_of(model, feats, flen, graphs, graph_of, big)
    x, hl = lg.double().cpu().numpy(), lens.cpu().numpy()
    ones = np.ones(B)
    num = R.logp_and_grad(x, hl, graphs, list(range(B)))
    den = P.logp_and_grad(x, hl, big, 12.0, fast=True)
    assert_insensitive(x, hl, big, 12.0, ones, den, grad=True, fast=True)
    check_logp(info["logp"].cpu().numpy(), num[0], "model: numerator")
    check_logp(info["logp_den"].cpu().numpy(), den[0], "model: denominator")
    # d loss = -(d num - 0.5 d den) / B: the tolerance of a gradient scaled by 1 / B (the larger of the two scales)
    check_grad(got.cpu().numpy(), -(num[1] - 0.5 * den[1]) / B, np.full(B, 1.0 / B), "model: num - 0.5 den")


def dlogits_of(model, feats, flen, graphs, graph_of, den):
    """d loss / d logits of ctc_graph_loss(denominator=..., den_scale=0.5)'s formula, with the CTC logits as the leaf."""
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        lens = mask.squeeze(1).sum(1)
        lg = model.ctc.logits(enc).clone()
    lg.requires_grad_(True)
    num = ops.ctc_graph_logp(lg, lens, graphs, graph_of)
    dn = ops.ctc_graph_beam_logp(lg, lens, den, 12.0)[0]
    (-(num - 0.5 * dn).sum() / lg.shape[0]).backward()
    return lg.grad, lg.detach(), lens
