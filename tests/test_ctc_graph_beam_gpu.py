"""GPU: beam-pruned CTC decoding over large token graphs (oe_ctc_graph_beam) through the C ABI, and through
ops.ctc_graph_beam_decode / ASRModel.ctc_graph_search(beam=...).

Three yardsticks.  (1) oe_ctc_graph itself: with beam = inf and max_active >= Q + A every shared output must EQUAL the dense
kernel's bit for bit, on grid values and on continuous raw logits, over the shapes test_ctc_graph_gpu.py uses for the dense
kernel's edges (they are built by its exact_case).  (2) The restatement (ctc_graph_beam_ref.py): on the 1/8 grid every float32
sum is exact, so with normalized=1 every output, status and peak must equal the float64 restatement bit for bit; on continuous
float32 log-probabilities they must equal the float32 restatement, which takes every sum and the threshold's subtraction in
the header's order.  (3) Raw mode on a large graph: the device's path must be one the graph accepts, its float64 rescoring
within the aligner's tolerance (rtol 1e-4 / atol 1e-3, as test_ctc_graph_gpu.py) of the float64 restatement of the same
pruned search.

The kernel runs 1024 threads per utterance and appends to its lists a wave at a time (survivor counts 63 / 64 / 65 and 1023 /
1024 / 1025), gives a node of more than 16 leaving arcs to a wave, and keeps arc and node ids in 32 bits (ids above 2^15 and
2^16; graphs just over each dense limit).  Every call's outputs and workspace carry guard elements behind them.

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_align_ref as AR  # noqa: E402
import ctc_graph_beam_ref as BR  # noqa: E402
import test_ctc_graph_gpu as G  # noqa: E402  (the dense kernel's cases, its Call and its replay; nothing of it is collected here)
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import MAX_ARCS, MAX_NODES, DecodingGraph  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3
SENT_I, SENT_F, SENT_B = -7, 5.0, 0xA5
GUARD = 64
NAMES = G.NAMES + ("status", "peak")
FLOATS = G.FLOATS
INF = float("inf")


class Call:
    """One oe_ctc_graph_beam call with its device buffers: sentinel-filled outputs with GUARD elements behind each, GUARD
    bytes behind the workspace; run() launches on the current stream."""

    def __init__(self, logits, hlens, g, beam, max_active=None, max_trav=None, normalized=True, ldv=None, want_logp=True):
        logits = torch.as_tensor(np.asarray(logits), dtype=torch.float32)
        B, T, V = logits.shape
        self.ldv = ldv or V
        self.buf = torch.full((B, T, self.ldv), 3.0, device=DEV)             # what lies behind V must not be read
        self.buf[:, :, :V] = logits.to(DEV)
        self.t = [torch.from_numpy(a).to(DEV) for a in g.host_tables() + g.host_out_tables()]
        self.graph = hip.BeamGraph(g.num_nodes, g.num_arcs, *(t.data_ptr() for t in self.t[:8]), len(g.cols), *(t.data_ptr() for t in self.t[8:]))
        self.hl = torch.as_tensor(np.asarray(hlens), dtype=torch.int32).to(DEV)
        self.max_active = g.num_nodes + g.num_arcs if max_active is None else max_active
        self.max_trav = T if max_trav is None else max_trav
        self.nbytes = hip.lib().oe_ctc_graph_beam_workspace_bytes(B, T, len(g.cols), g.num_nodes, g.num_arcs, self.max_active)
        assert self.nbytes > 0
        self.ws = torch.full((self.nbytes + GUARD,), SENT_B, dtype=torch.uint8, device=DEV)
        self.shape, self.want_logp = (B, T, V), want_logp
        a = self.args = hip.CtcGraphBeamArgs()
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = self.buf.data_ptr(), self.ldv, B, T, V, self.hl.data_ptr()
        a.graph, a.normalized, a.max_trav, a.max_active, a.beam = C.pointer(self.graph), int(normalized), self.max_trav, self.max_active, beam
        a.workspace = self.ws.data_ptr()
        self.fresh_outputs()

    def fresh_outputs(self):
        B, T, _ = self.shape
        M, lg = self.max_trav, self.want_logp
        shapes = [(B,), (B, T), (B, T), (B, T) if lg else None, (B,), (B, M), (B, M), (B, M), (B, M) if lg else None, (B,), (B,)]
        self.flat, self.out = [], []
        for name, shape in zip(NAMES, shapes):
            if shape is None:
                self.flat.append(None)
                self.out.append(None)
                continue
            f = name in FLOATS
            flat = torch.full((int(np.prod(shape)) + GUARD,), SENT_F if f else SENT_I, dtype=torch.float32 if f else torch.int32, device=DEV)
            self.flat.append(flat)
            self.out.append(flat[:-GUARD].view(shape))
        a = self.args
        (a.score, a.frames, a.arcs, a.path_logp, a.n_trav, a.trav_arc, a.trav_start, a.trav_end, a.trav_logp, a.status, a.peak) = (
            None if t is None else t.data_ptr() for t in self.out)

    def launch(self):
        return hip.lib().oe_ctc_graph_beam(C.byref(self.args), hip.stream())

    def run(self):
        hip.check(self.launch(), "oe_ctc_graph_beam")
        torch.cuda.synchronize()
        assert self.guards_intact()
        return self.numpy()

    def numpy(self):
        return [None if t is None else t.cpu().numpy() for t in self.out]

    def guards_intact(self):
        tails = all(bool((f[-GUARD:] == (SENT_I if f.dtype == torch.int32 else SENT_F)).all()) for f in self.flat if f is not None)
        return tails and bool((self.ws[self.nbytes:] == SENT_B).all())

    def untouched(self):
        return self.guards_intact() and all(bool((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all()) for t in self.out if t is not None)


def stack(per, dtype_of_floats=np.float32):
    """Restatement results of a batch, stacked and cast to the device's dtypes (exact on the grid)."""
    return [np.stack([np.asarray(p[name]) for p in per]).astype(dtype_of_floats if name in FLOATS else np.int32) for name in NAMES]


def assert_equal_outputs(got, want, names=NAMES):
    for name, g, w in zip(names, got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist(), g[g != w][:5], w[g != w][:5])


def grid(rng, n, lo):
    return rng.integers(8 * lo, 1, size=n).astype(np.float64) / 8


# ---------------------------------------------------------------- 1: beam = inf against oe_ctc_graph
DENSE_EDGES = ["A1023", "A1024", "A1025", "in_degree_32", "in_degree_33", "in_degree_63", "in_degree_64", "in_degree_65", "in_degree_1500",
               "T1", "T2", "T3", "hlens_0_1_T", "self_loops", "parallel_arcs_equal_labels", "labels_outside_the_vocabulary", "B3_ragged",
               "no_reachable_final", "ldv_wider_than_V"]


@pytest.mark.parametrize("name", DENSE_EDGES)
def test_without_a_beam_every_shared_output_equals_the_dense_kernel_bit_for_bit(name):
    c = G.exact_case(name)
    g = c["g"]
    rng = np.random.default_rng(len(name))
    raw = rng.standard_normal(c["lp"].shape).astype(np.float32) * 3
    for logits, normalized in ((c["lp"], True), (raw, False)):
        want = G.Call(logits, c["hlens"], g, c["max_trav"], normalized, ldv=c["ldv"]).run()
        got = Call(logits, c["hlens"], g, INF, None, c["max_trav"], normalized, ldv=c["ldv"]).run()
        assert_equal_outputs(got[:9], want, G.NAMES)
        for f in (0, 3, 8):                                                  # the floats in every bit, the zero's sign included
            assert got[f].tobytes() == want[f].tobytes(), G.NAMES[f]
        feasible = np.isfinite(want[0])
        assert np.array_equal(got[9], np.where(feasible, BR.OK, BR.INFEASIBLE).astype(np.int32))
        assert (got[10] <= g.num_nodes + g.num_arcs).all() and ((got[10] > 0) == (np.minimum(np.asarray(c["hlens"]), c["T"]) > 0)).all()
        print(f"{name} normalized={normalized}: Q={g.num_nodes} A={g.num_arcs} score {want[0].tolist()} peak {got[10].tolist()}")
    # the optional outputs are optional: without them the rest is the same
    bare = Call(c["lp"], c["hlens"], g, INF, None, c["max_trav"], True, ldv=c["ldv"], want_logp=False).run()
    assert bare[3] is None and bare[8] is None
    assert_equal_outputs(bare[:9], G.Call(c["lp"], c["hlens"], g, c["max_trav"], True, ldv=c["ldv"]).run(), G.NAMES)


# ---------------------------------------------------------------- 2: finite beams against the restatement
def two_words():
    return DecodingGraph(4, [(0, 1, 1, 0.0), (1, 3, 2, 0.0), (0, 2, 3, 0.0), (2, 3, 4, 0.0)], {3: 0.0})


@functools.lru_cache(maxsize=None)
def finite_case(name):
    """-> (g, lp (B, T, V) float64 on the grid, hlens, the beams: 0, one that puts a state exactly on a threshold, a wide one)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "two_words":                                                  # test_ctc_graph_beam_ref.py works these out by hand
        lp = np.full((1, 4, 5), -8.0)
        lp[0, 0, 1], lp[0, 0, 3], lp[0, 1, 1], lp[0, 1, 3] = -1.0, -2.0, -1.0, -1.0
        lp[0, 2:, 2], lp[0, 2:, 4] = -3.0, -0.5
        return two_words(), lp, [4], (0.0, 1.0, 0.875, 12.0)
    if name == "final_state_pruned":
        g = DecodingGraph(3, [(0, 1, 1, 0.0), (0, 2, 2, 0.0)], {2: 0.0})
        return g, np.array([[[-8.0, -0.125, -6.0], [-0.125, -0.125, -0.125]]]), [2], (0.0, 5.875, 7.0)
    if name == "random_40":
        g = DecodingGraph(40, G.random_arcs(rng, 40, 300, 6), G.random_finals(rng, 40))
        return g, grid(rng, (3, 16, 6), -8), [16, 9, 1], (0.0, 2.0, 9.0)
    if name == "fan_in_65":
        return G.fan_in(rng, 65, 6), grid(rng, (2, 20, 6), -8), [20, 13], (0.0, 1.5, 10.0)
    if name == "looped_trie":
        phrases = list(dict.fromkeys(tuple(int(t) for t in rng.integers(1, 30, size=int(rng.integers(2, 5)))) for _ in range(400)))[:300]
        g = DecodingGraph.from_phrases(phrases, weights=grid(rng, len(phrases), -2).tolist(), loop=True)
        return g, grid(rng, (2, 24, 30), -8), [24, 17], (0.0, 3.0, 14.0)
    raise KeyError(name)


FINITE = ["two_words", "final_state_pruned", "random_40", "fan_in_65", "looped_trie"]


@functools.lru_cache(maxsize=None)
def finite_ref(name, beam, f32):
    g, lp, hlens, _ = finite_case(name)
    dt = np.float32 if f32 else np.float64
    return [BR.decode_graph(soften(lp[b]) if f32 else lp[b], hlens[b], g, beam, None, dt) for b in range(len(hlens))]


def soften(lp):
    """Continuous float32 log-probabilities from a grid case: the grid values off the grid."""
    return (lp * np.float64(1.0379) - np.float64(0.0131) * np.arange(lp.shape[-1])).astype(np.float32)


@pytest.mark.parametrize("name,which", [(n, i) for n in FINITE for i in range(len(finite_case(n)[3]))])
def test_a_finite_beam_equals_the_restatement_bit_for_bit(name, which):
    g, lp, hlens, beams = finite_case(name)
    beam = beams[which]
    for f32 in (False, True):                                                # the grid in float64; continuous values in float32
        per = finite_ref(name, beam, f32)
        x = np.stack([soften(lp[b]) for b in range(len(hlens))]) if f32 else lp
        got = Call(x, hlens, g, beam).run()
        assert_equal_outputs(got, stack(per))
        if f32:
            for f in (0, 3, 8):
                assert got[f].tobytes() == stack(per)[f].tobytes(), NAMES[f]
        print(f"{name} beam {beam} {'float32' if f32 else 'grid'}: pruned {[sum(p['pruned']) for p in per]} at thr "
              f"{[sum(p['at_thr']) for p in per]} peak {[p['peak'] for p in per]} status {[p['status'] for p in per]}")
        assert sum(sum(p["pruned"]) for p in per) >= 1                       # the case prunes


def test_the_finite_beam_cases_are_not_vacuous():
    changed = lost = on_thr = 0
    for name in FINITE:
        g, lp, hlens, beams = finite_case(name)
        free = finite_ref(name, INF, False)
        assert beams[0] == 0.0 and beams[-1] >= 7.0
        assert sum(sum(p["at_thr"]) for p in finite_ref(name, beams[1], False)) >= 1, name       # a state exactly on a threshold survives
        for beam in beams:
            for p, f in zip(finite_ref(name, beam, False), free):
                if p["status"] == BR.OK and not np.array_equal(p["frames"], f["frames"]):
                    assert p["score"] < f["score"]
                    changed += 1
                if p["status"] == BR.INFEASIBLE and f["status"] == BR.OK:
                    lost += 1
                on_thr += sum(p["at_thr"])
    print(f"{changed} pruned paths differ from the unpruned ones, {lost} utterances infeasible through pruning alone, {on_thr} states on a threshold")
    assert changed >= 1 and lost >= 1


# ---------------------------------------------------------------- 3: capacity
def capacity_graph(N):
    """A star whose survivor counts are K + 1 + e, then 2 K + 1 + e = N: K arcs of one label from node 0 to K nodes, and for an
    even N a self-loop of another label at node 0 (e = 1)."""
    K, e = (N - 1) // 2, 1 - N % 2
    arcs = [(0, 1 + i, 1, 0.0) for i in range(K)] + [(0, 0, 2, 0.0)] * e
    return DecodingGraph(K + 1, arcs, {1: 0.0, 0: -1.0}), K + 1 + e


@pytest.mark.parametrize("N", [63, 64, 65, 1023, 1024, 1025])
def test_exactly_max_active_survivors_decode_and_one_more_overflows(N):
    g, first = capacity_graph(N)
    lp = np.full((2, 3, 3), -1.0)
    lp[1, :, 1] = -0.5
    hlens = [3, 2]
    free = [BR.decode_graph(lp[b], hlens[b], g) for b in range(2)]
    assert [p["survivors"] for p in free] == [[first, N, N], [first, N]]
    for beam in (INF, 4.0):
        fits = Call(lp, hlens, g, beam, max_active=N)
        assert_equal_outputs(fits.run(), stack([BR.decode_graph(lp[b], hlens[b], g, beam, N) for b in range(2)]))
        assert (fits.numpy()[9] == BR.OK).all() and (fits.numpy()[10] == N).all()
        over = Call(lp, hlens, g, beam, max_active=N - 1)
        got = over.run()                                                      # run() checks the guards behind every buffer
        assert_equal_outputs(got, stack([BR.decode_graph(lp[b], hlens[b], g, beam, N - 1) for b in range(2)]))
        assert (got[9] == BR.OVERFLOW).all() and (got[10] == N).all()
        assert np.isneginf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all() and (got[3] == 0).all() and (got[4] == 0).all()
        assert (got[5] == -1).all() and (got[6] == -1).all() and (got[7] == -1).all() and (got[8] == 0).all()
    small = Call(lp, hlens, g, INF, max_active=first - 1).run()               # the FIRST overflowing frame's count
    assert (small[9] == BR.OVERFLOW).all() and (small[10] == first).all()
    one = Call(lp, [3, 0], g, INF, max_active=N - 1).run()                    # an utterance's overflow is its own
    assert one[9].tolist() == [BR.OVERFLOW, BR.INFEASIBLE] and one[10].tolist() == [N, 0]


# ---------------------------------------------------------------- 4, 5: beyond the dense limits
@functools.lru_cache(maxsize=None)
def lexicon():
    """A looped trie of 70000 four-token words over 89 tokens with a unigram weight each: more than 2^16 nodes, more than 2^15
    arcs into node 0; three utterances of at most 12 frames that speak a word or two over grid noise."""
    rng = np.random.default_rng(41)
    V, T = 90, 12
    words = np.unique(rng.integers(1, V, size=(76000, 4)), axis=0)
    words = words[(np.diff(words, axis=1) != 0).all(axis=1)][:70000]          # no repeated token: a word fits four frames
    assert len(words) == 70000
    g = DecodingGraph.from_phrases(words.tolist(), weights=grid(rng, len(words), -2).tolist(), loop=True, large=True)
    assert g.num_nodes > 1 << 16 and int(np.diff(g.in_ptr)[0]) > 1 << 15 and g.num_arcs > MAX_ARCS
    lp = grid(rng, (3, T, V), -8) - 2.0
    hlens = [12, 9, 5]
    for b, (first, second) in enumerate(((11, 40000), (69999, 3), (123, None))):
        t = 0
        for wd in (first, second):
            if wd is not None and t + 4 <= hlens[b]:
                lp[b, np.arange(t, t + 4), words[wd]] = -0.125
                t += 5
    return g, words, lp, hlens


@pytest.mark.parametrize("beam,max_active", [(INF, None), (6.0, 32768), (2.0, 4096)])
def test_a_lexicon_loop_beyond_every_dense_limit_equals_the_restatement(beam, max_active):
    g, words, lp, hlens = lexicon()
    per = [BR.decode_graph(lp[b], hlens[b], g, beam, max_active) for b in range(3)]
    got = Call(lp, hlens, g, beam, max_active).run()
    print(f"lexicon Q={g.num_nodes} A={g.num_arcs} beam {beam}: score {[p['score'] for p in per]} peak {[p['peak'] for p in per]} "
          f"pruned {[sum(p['pruned']) for p in per]} highest arc on a path {int(got[2].max())}")
    assert_equal_outputs(got, stack(per))
    assert per[1]["status"] == per[2]["status"] == BR.OK and int(got[2].max()) > 1 << 15
    assert per[0]["status"] == (BR.OK if beam >= 6.0 else BR.INFEASIBLE)    # the narrow beam loses the first utterance: status 1, not 2
    if per[0]["status"] == BR.OK:
        assert AR.collapse(per[0]["frames"][: hlens[0]])[:4] == words[11].tolist()
    if beam < INF:
        assert all(sum(p["pruned"]) > 0 for p in per) and max(p["peak"] for p in per) < (g.num_nodes + g.num_arcs) // 4


def chain_with_branches(Q, A):
    """Nodes 0 .. Q-1 in a chain, every node final, and A - (Q - 1) more arcs: skips and parallel arcs near the start."""
    rng = np.random.default_rng(Q + A)
    extra = A - (Q - 1)
    src = np.concatenate((np.arange(Q - 1), rng.integers(0, 6, extra)))
    dst = np.concatenate((np.arange(1, Q), src[Q - 1:] + rng.integers(0, 3, extra)))
    lab = np.concatenate((1 + np.arange(Q - 1) % 5, rng.integers(1, 6, extra)))
    return DecodingGraph.from_arrays(Q, src, dst, lab, grid(rng, A, -3), grid(rng, Q, -3), large=True)


@pytest.mark.parametrize("Q,A", [(MAX_NODES + 1, 12000), (5000, MAX_ARCS + 1), (MAX_NODES + 1, MAX_ARCS + 1)])
def test_a_graph_just_over_a_dense_limit(Q, A):
    g = chain_with_branches(Q, A)
    rng = np.random.default_rng(Q)
    lp, hlens = grid(rng, (2, 10, 6), -8), [10, 6]
    for beam in (INF, 3.0):
        per = [BR.decode_graph(lp[b], hlens[b], g, beam) for b in range(2)]
        assert_equal_outputs(Call(lp, hlens, g, beam).run(), stack(per))
        assert all(p["status"] == BR.OK for p in per) and (beam == INF or all(sum(p["pruned"]) > 0 for p in per))


def test_raw_mode_on_the_lexicon_loop():
    g, words, grid_lp, hlens = lexicon()
    rng = np.random.default_rng(43)
    logits = rng.standard_normal(grid_lp.shape).astype(np.float32) * 1.5
    logits += (grid_lp > -1).astype(np.float32) * 6.0                        # the same words, spoken over continuous noise
    beam, max_active = 6.0, 1 << 17
    got = Call(logits, hlens, g, beam, max_active, normalized=False).run()
    score, frames, arcs, path_logp, n_trav, ta, ts, te, tl, status, peak = got
    for b in range(3):
        lp64 = AR.log_softmax(logits[b])
        ref = BR.decode_graph(lp64, hlens[b], g, beam, max_active)
        assert status[b] == BR.OK == ref["status"] and sum(ref["pruned"]) > 0
        mine = G.replay(g, lp64, hlens[b], frames[b], arcs[b], int(n_trav[b]), ta[b], ts[b], te[b])      # asserts g.accepts(frames)
        print(f"utterance {b}: restatement {ref['score']:.6f}, device {score[b]:.6f}, its path rescored {mine:.6f}, peak {peak[b]} / {ref['peak']}")
        np.testing.assert_allclose(mine, ref["score"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(score[b], ref["score"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(path_logp[b, : hlens[b]], lp64[np.arange(hlens[b]), frames[b, : hlens[b]]], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------- 6: determinism and independence
def test_two_runs_one_utterance_alone_and_a_captured_replay_agree():
    g, lp, hlens, beams = finite_case("looped_trie")
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((3, 24, 30)).astype(np.float32) * 3
    hlens = [24, 17, 20]
    call = Call(logits, hlens, g, 5.0, 4096, normalized=False)
    first = call.run()
    assert (first[9] == BR.OK).all() and (first[10] < g.num_nodes + g.num_arcs).all()
    call.fresh_outputs()
    assert_equal_outputs(call.run(), first)
    for b in range(3):
        alone = Call(logits[b: b + 1], hlens[b: b + 1], g, 5.0, 4096, normalized=False).run()
        assert_equal_outputs(alone, [x[b: b + 1] for x in first])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.check(call.launch(), "oe_ctc_graph_beam")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            hip.check(call.launch(), "oe_ctc_graph_beam")
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for _ in range(2):
        for t in call.out:
            t.fill_(SENT_I if t.dtype == torch.int32 else SENT_F)
        torch.cuda.synchronize()
        assert call.untouched()
        graph.replay()
        torch.cuda.synchronize()
        assert call.guards_intact()
        assert_equal_outputs(call.numpy(), first)


# ---------------------------------------------------------------- 7: contract
@pytest.mark.parametrize("what,text", [
    ("Q0", b"Q=0"), ("Qbig", b"Q=1048577"), ("A0", b"A=0"), ("Abig", b"A=4194305"), ("U0", b"U=0"), ("UV", b"U=6"), ("B0", b"B=0"),
    ("T0", b"T=0"), ("Tbig", b"T=1048577"), ("V1", b"V=1"), ("ldv", b"ldv=5"), ("max_trav", b"max_trav=0"), ("max_active", b"max_active=0"),
    ("beam_negative", b"beam=-1"), ("beam_nan", b"beam=nan"), ("logits", b"logits"), ("hlens", b"hlens"), ("graph", b"graph"),
    ("workspace", b"workspace"), ("misaligned", b"aligned"), ("score", b"output"), ("frames", b"output"), ("arcs", b"output"),
    ("n_trav", b"output"), ("trav_arc", b"output"), ("trav_start", b"output"), ("trav_end", b"output"), ("status", b"output"),
    ("peak", b"output"), ("in_ptr", b"table"), ("src", b"table"), ("dst", b"table"), ("label", b"table"), ("col", b"table"), ("w", b"table"),
    ("final", b"table"), ("cols", b"table"), ("out_ptr", b"table"), ("out_arc", b"table")])
def test_bad_arguments_leave_the_outputs_untouched(what, text):
    c = G.exact_case("self_loops")
    call = Call(c["lp"], c["hlens"], c["g"], 2.0, 64, 4)
    a, g = call.args, call.graph
    if what in ("Q0", "Qbig"):
        g.Q = 0 if what == "Q0" else (1 << 20) + 1
    elif what in ("A0", "Abig"):
        g.A = 0 if what == "A0" else (1 << 22) + 1
    elif what in ("U0", "UV"):
        g.U = 0 if what == "U0" else c["V"]
    elif what == "B0":
        a.B = 0
    elif what in ("T0", "Tbig"):
        a.T = 0 if what == "T0" else (1 << 20) + 1
    elif what == "V1":
        a.V = 1
    elif what == "ldv":
        a.ldv = 5
    elif what in ("max_trav", "max_active"):
        setattr(a, what, 0)
    elif what.startswith("beam_"):
        a.beam = -1.0 if what == "beam_negative" else float("nan")
    elif what == "graph":
        a.graph = None
    elif what == "misaligned":
        a.workspace = call.ws.data_ptr() + 4
    elif what in ("logits", "hlens", "workspace", "score", "frames", "arcs", "n_trav", "trav_arc", "trav_start", "trav_end", "status", "peak"):
        setattr(a, what, None)
    else:
        setattr(g, what, None)
    lib = hip.lib()
    rc = call.launch()
    assert rc != 0 and text in lib.oe_last_error(), lib.oe_last_error()
    torch.cuda.synchronize()
    assert call.untouched()


def test_workspace_bytes_follow_the_documented_formula():
    f = hip.lib().oe_ctc_graph_beam_workspace_bytes
    up4, up16 = lambda x: (x + 3) // 4 * 4, lambda x: (x + 15) // 16 * 16

    def formula(B, T, U, Q, A, max_active):
        M = up4(min(max_active, Q + A))
        return up16(4 * B * T * (U + 1)) + B * (40 * up4(Q) + 20 * up4(A) + 28 * M + 8 * T * M)
    for shape in ((2, 10, 3, 5, 9, 4), (2, 10, 3, 5, 9, 1000), (3, 7, 2, 1, 1, 1), (1, 1 << 20, 1, 1 << 20, 1 << 22, 16384), (5, 300, 5000, 400000, 500000, 1 << 15)):
        assert f(*shape) == formula(*shape), shape
    # the graph's size is paid once, not per frame: ten times the frames cost ten times the lists and rows, not the graph
    assert f(1, 1000, 1, 1 << 20, 1 << 22, 1024) - f(1, 100, 1, 1 << 20, 1 << 22, 1024) == 900 * (8 * 1024 + 8)
    for bad in ((0, 10, 3, 5, 9, 4), (2, 0, 3, 5, 9, 4), (2, (1 << 20) + 1, 3, 5, 9, 4), (2, 10, 0, 5, 9, 4), (2, 10, 3, 0, 9, 4),
                (2, 10, 3, (1 << 20) + 1, 9, 4), (2, 10, 3, 5, 0, 4), (2, 10, 3, 5, (1 << 22) + 1, 4), (2, 10, 3, 5, 9, 0), (-1, 10, 3, 5, 9, 4)):
        assert f(*bad) == 0, bad
    assert hip.lib().oe_abi_version() >= 9


# ---------------------------------------------------------------- 8: python layers
def test_ops_utterance_groups_equal_the_one_call_result():
    from openeat_amd import ops
    g, lp, hlens, beams = finite_case("random_40")
    B, T, V = lp.shape
    lg, hl = torch.from_numpy(lp.astype(np.float32)).to(DEV), torch.tensor(hlens, device=DEV)
    whole = ops.ctc_graph_beam_decode(lg, hl, g, 2.0, normalized=True)
    per_utt = hip.lib().oe_ctc_graph_beam_workspace_bytes(1, T, len(g.cols), g.num_nodes, g.num_arcs, 16384)
    parts = ops.ctc_graph_beam_decode(lg, hl, g, 2.0, normalized=True, workspace_cap=per_utt)           # three groups of one
    pairs = ops.ctc_graph_beam_decode(lg, hl, g, 2.0, normalized=True, workspace_cap=2 * per_utt + 40)  # two and one
    torch.cuda.synchronize()
    assert len(whole) == 11
    assert_equal_outputs([t.cpu().numpy() for t in whole], stack(finite_ref("random_40", 2.0, False)))
    for name, a, b, d in zip(NAMES, whole, parts, pairs):
        assert a.dtype == b.dtype and torch.equal(a, b) and torch.equal(a, d), name
    tight = ops.ctc_graph_beam_decode(lg, hl, g, INF, max_active=30, normalized=True)
    assert_equal_outputs([t.cpu().numpy() for t in tight], stack([BR.decode_graph(lp[b], hlens[b], g, INF, 30) for b in range(B)]))
    assert tight[9].tolist() == [BR.OVERFLOW, BR.OVERFLOW, BR.OK] and tight[10][2].item() <= 30 < tight[10][0].item()
    with pytest.raises(TypeError):
        ops.ctc_graph_beam_decode(lg, hl, [[1, 2]], 2.0)
    for bad in (dict(beam=-1.0), dict(beam=float("nan")), dict(beam=2.0, max_active=0), dict(beam=2.0, max_trav=0)):
        with pytest.raises(ValueError):
            ops.ctc_graph_beam_decode(lg, hl, g, **bad)
    with pytest.raises(ValueError):
        ops.ctc_graph_beam_decode(lg, hl, DecodingGraph.linear([]), 2.0)      # a graph without arcs has no device form


def test_model_graph_search_with_a_beam(monkeypatch):
    from openeat_amd import ops
    model, i = G.tiny_conformer()
    feats, flen = i["feats"][:2], i["flen"][:2]
    V = model.vocab_size
    loop = DecodingGraph.token_loop(V - 1)                                   # U = V - 2 < V
    dense = model.ctc_graph_search(feats, flen, loop)
    assert all(r.feasible and len(r.tokens) >= 2 for r in dense)
    free = model.ctc_graph_search(feats, flen, loop, beam=INF)
    for a, b in zip(dense, free):
        assert (a.tokens, a.score, a.traversals) == (b.tokens, b.score, b.traversals)
    # max_active 2 overflows (a token loop keeps node 0 and every arc alive): the utterances run again, doubled, until they fit
    asked = []
    real = ops.ctc_graph_beam_decode
    monkeypatch.setattr(ops, "ctc_graph_beam_decode", lambda *a, **k: asked.append((a[0].shape[0], a[4])) or real(*a, **k))
    again = model.ctc_graph_search(feats, flen, loop, beam=INF, max_active=2, with_times=True)
    assert [r.tokens for r in again] == [r.tokens for r in dense] and [r.score for r in again] == [r.score for r in dense]
    assert asked == [(2, 2), (2, loop.num_nodes + loop.num_arcs)]            # frame 0 already has every state alive: from its peak
    assert "start_s" in again[0].traversals[0]
    narrow = model.ctc_graph_search(feats, flen, loop, beam=0.0)             # beam 0 keeps the best state of every frame: the same path here
    assert [r.tokens for r in narrow] == [r.tokens for r in dense]
    # ... and when one utterance's workspace would exceed the cap, the search says which utterance and how many states it had
    T = model.ctc_logits_windowed(feats, flen, None, 16)[0].shape[1]
    cap = hip.lib().oe_ctc_graph_beam_workspace_bytes(2, T, len(loop.cols), 1, loop.num_arcs, 2)
    with pytest.raises(RuntimeError, match=r"utterance \d+ keeps \d+ states"):
        model.ctc_graph_search(feats, flen, loop, beam=INF, max_active=2, workspace_cap=cap)
    with pytest.raises(ValueError, match="max_active"):
        model.ctc_graph_search(feats, flen, loop, max_active=8)
    big = chain_with_branches(MAX_NODES + 1, 12000)
    with pytest.raises(ValueError, match="posterior"):
        model.ctc_graph_search(feats, flen, big, beam=4.0, posterior=True)
    with pytest.raises(ValueError):
        model.ctc_graph_search(feats, flen, big)                             # the dense search does not take it
    res = model.ctc_graph_search(feats, flen, big, beam=8.0)                 # the beam search does (every node is final)
    assert len(res) == 2 and all(r.feasible for r in res)
    # a chain's active set grows frame by frame: a small capacity is doubled several times, and the result is the same
    asked.clear()
    grown = model.ctc_graph_search(feats, flen, big, beam=8.0, max_active=16)
    assert [(r.tokens, r.score) for r in grown] == [(r.tokens, r.score) for r in res]
    print("capacities asked for:", asked)
    assert asked[0] == (2, 16) and len(asked) >= 3 and all(b[1] >= 2 * a[1] for a, b in zip(asked, asked[1:]))
