"""GPU: n-best grammar-constrained CTC decoding (oe_ctc_graph_nbest) through the C ABI against the restatement
(ctc_graph_nbest_ref.py), and through ops.ctc_graph_nbest / ASRModel.ctc_graph_search / ASRModel.graph_attention_rescoring.

Exact mode (normalized=1): log-probabilities, weights and final weights on the 1/8 grid, where every float32 sum is exact and
equal scores really tie, so every output must EQUAL the float32 restatement bit for bit, unused slots and sentinel-prefilled
outputs included.  The restatement runs with the device's hash as history identity and asserts on the way that no two
histories it meets share a hash: hash identity is tuple identity on every case here.  Raw mode (normalized=0): continuous
logits; the hypotheses are held to the float64 restatement where its scores are far enough apart to rank (asserted on the
reference alone), and each score to the float64 best-alignment score of its own path within the aligner's tolerance (rtol
1e-4 / atol 1e-3, as test_ctc_graph_gpu.py).

The kernel runs 1024 threads per utterance (A = 1023, 1024, 1025), gives a node of more than 32 incoming arcs to a wave
(in-degree 32, 33, 64, 65, 2000) and instantiates list capacities 1, 2, 4, 8 (K = 1, 2, 3, 8).

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_align_ref as AR  # noqa: E402
import ctc_graph_nbest_ref as N  # noqa: E402
import ctc_graph_ref as R  # noqa: E402
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import MAX_ARCS, MAX_NODES, DecodingGraph  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3
SENT_I, SENT_F = -7, 5.0
NAMES = ("n_hyp", "hyp_score", "hyp_len", "hyp_arcs", "hyp_tokens")
MODES = {"arcs": N.ARCS, "tokens": N.TOKENS}


class Call:
    """One oe_ctc_graph_nbest call with its device buffers: sentinel-filled outputs, run() launches on the current stream."""

    def __init__(self, logits, hlens, g, K, distinct, max_len, normalized, ldv=None):
        logits = torch.as_tensor(np.asarray(logits), dtype=torch.float32)
        B, T, V = logits.shape
        self.ldv = ldv or V
        self.buf = torch.full((B, T, self.ldv), 3.0, device=DEV)             # what lies behind V must not be read
        self.buf[:, :, :V] = logits.to(DEV)
        self.t = [torch.from_numpy(a).to(DEV) for a in g.host_tables()]
        in_ptr, src, dst, label, col, w, final, cols = self.t
        self.graph = hip.DecodingGraph(g.num_nodes, g.num_arcs, in_ptr.data_ptr(), src.data_ptr(), dst.data_ptr(), label.data_ptr(),
                                       col.data_ptr(), w.data_ptr(), final.data_ptr(), cols.data_ptr(), len(g.cols))
        self.hl = torch.as_tensor(np.asarray(hlens), dtype=torch.int32).to(DEV)
        nbytes = hip.lib().oe_ctc_graph_nbest_workspace_bytes(B, T, len(g.cols), g.num_nodes, g.num_arcs, K)
        assert nbytes == workspace_formula(B, T, len(g.cols), g.num_nodes, g.num_arcs, K)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.shape, self.K, self.max_len = (B, T, V), K, max_len
        a = self.args = hip.CtcGraphNbestArgs()
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = self.buf.data_ptr(), self.ldv, B, T, V, self.hl.data_ptr()
        a.graph, a.normalized, a.nbest, a.distinct, a.max_len = C.pointer(self.graph), int(normalized), K, MODES[distinct], max_len
        a.workspace = self.ws.data_ptr()
        self.fresh_outputs()

    def fresh_outputs(self):
        B, K, M = self.shape[0], self.K, self.max_len
        i32 = lambda *s: torch.full(s, SENT_I, dtype=torch.int32, device=DEV)
        self.out = [i32(B), torch.full((B, K), SENT_F, dtype=torch.float32, device=DEV), i32(B, K), i32(B, K, M), i32(B, K, M)]
        a = self.args
        a.n_hyp, a.hyp_score, a.hyp_len, a.hyp_arcs, a.hyp_tokens = (t.data_ptr() for t in self.out)

    def launch(self):
        return hip.lib().oe_ctc_graph_nbest(C.byref(self.args), hip.stream())

    def run(self):
        hip.check(self.launch(), "oe_ctc_graph_nbest")
        torch.cuda.synchronize()
        return self.numpy()

    def numpy(self):
        return [t.cpu().numpy() for t in self.out]

    def untouched(self):
        return all(bool((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all()) for t in self.out)


def workspace_formula(B, T, U, Q, A, K):
    """The header's: 16-byte tokens (the double-buffered lists, the per-node lists), then 4-byte words, rounded up to 16."""
    words = B * (K * Q + T * A * K + T * (U + 1))
    return 16 * B * K * (2 * A + 2 * Q + K * Q) + (words + 3) // 4 * 16


def reference(lp, hlens, g, K, distinct, max_len, dtype=np.float32):
    """The restatement of a batch with hash identity (and the check that no two histories share a hash), stacked."""
    per = [N.nbest_graph(lp[b], hlens[b], g, K, MODES[distinct], dtype, "hash", max_len, keys_seen={}) for b in range(len(hlens))]
    return [np.stack([np.asarray(p[name]) for p in per]).astype(np.float32 if name == "hyp_score" else np.int32) for name in NAMES], per


def assert_equal_outputs(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist(), g[g != w][:5], w[g != w][:5])


# ---------------------------------------------------------------- exact mode
def grid(rng, n, lo):
    return rng.integers(8 * lo, 1, size=n).astype(np.float64) / 8


def random_arcs(rng, Q, A, V, near_start=0.3):
    """A arcs over Q nodes; a share of them leaves the first few nodes so that much of the graph is reachable in a few frames."""
    src = np.where(rng.random(A) < near_start, rng.integers(0, min(Q, 4), size=A), rng.integers(0, Q, size=A))
    return [(int(s), int(d), int(c), float(w)) for s, d, c, w in zip(src, rng.integers(0, Q, size=A), rng.integers(1, V, size=A), grid(rng, A, -4))]


def random_finals(rng, Q):
    return {int(q): float(grid(rng, 1, -4)[0]) for q in rng.integers(0, Q, size=max(Q // 2, 1))}


def fan_in(rng, d, V):
    """Node 1 has d incoming arcs (from 0, 2 and 3, itself included when d is large), and arcs of every label leave it: each
    selects over the d arcs of another label."""
    arcs = [(int(rng.choice([0, 2, 3, 1] if d > 8 else [0, 2, 3])), 1, int(c), float(w))
            for c, w in zip(rng.integers(1, V, size=d), grid(rng, d, -4))]
    arcs += [(1, int(rng.integers(2, 4)), c, float(grid(rng, 1, -4)[0])) for c in range(1, V)]
    arcs += [(0, int(rng.integers(2, 4)), int(rng.integers(1, V)), 0.0) for _ in range(3)]
    return DecodingGraph(4, arcs, {2: -0.5, 3: 0.0, 1: -1.0})


def exact_case(name):
    """-> dict(lp (B, T, V) float64 on the 1/8 grid, hlens, g, max_len, ldv)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    c = dict(B=1, T=8, V=6, max_len=None, ldv=None)
    if name == "Q1_A1":
        c.update(g=DecodingGraph(1, [(0, 0, 2, -0.5)], {0: -0.25}))
    elif name.startswith("in_degree_"):
        d = int(name.split("_")[2])
        c.update(g=fan_in(rng, d, c["V"]), T=4 if d >= 1000 else 8)
    elif name in ("A1023", "A1024", "A1025"):
        c.update(g=DecodingGraph(200, random_arcs(rng, 200, int(name[1:]), 6), random_finals(rng, 200)), T=6)
    elif name == "A_max":
        c.update(g=DecodingGraph(4096, random_arcs(rng, 4096, MAX_ARCS, 9, near_start=0.02), random_finals(rng, 4096)), T=4, V=9)
    elif name == "Q_max":
        c.update(g=DecodingGraph(MAX_NODES, random_arcs(rng, MAX_NODES, 10000, 9, near_start=0.03), random_finals(rng, MAX_NODES)), T=4, V=9)
    elif name == "self_loops":
        c.update(g=DecodingGraph(2, [(0, 0, 1, -0.125), (0, 0, 2, 0.0), (0, 1, 3, -0.5), (1, 1, 3, 0.0), (1, 1, 1, -0.25), (1, 0, 4, 0.0)],
                                 {1: 0.0, 0: -1.0}))
    elif name == "parallel_arcs_equal_labels":
        c.update(g=DecodingGraph(3, [(0, 1, 2, -1.0), (0, 1, 2, -0.25), (0, 1, 2, -0.25), (1, 2, 3, -0.5), (1, 2, 3, 0.0), (1, 2, 2, 0.0)],
                                 {2: 0.0}))
    elif name == "same_src_and_label_two_dst":
        c.update(g=DecodingGraph(4, [(0, 1, 2, 0.0), (0, 2, 2, 0.0), (1, 3, 3, -0.5), (2, 3, 4, -0.25), (2, 0, 1, 0.0), (2, 3, 3, -0.5)], {3: 0.0}))
    elif name == "unreachable_node":
        c.update(g=DecodingGraph(5, [(0, 1, 1, 0.0), (1, 2, 2, 0.0), (3, 2, 4, 0.0), (3, 4, 1, 0.0), (4, 3, 2, 0.0), (2, 1, 5, -0.5)],
                                 {2: 0.0, 4: 0.0}))
    elif name == "no_reachable_final":
        c.update(g=DecodingGraph(4, [(0, 1, 1, 0.0), (1, 0, 2, 0.0), (3, 2, 4, 0.0), (2, 2, 1, 0.0)], {2: 0.0, 3: -1.0}))
    elif name == "empty_path":
        c.update(g=DecodingGraph(2, [(0, 1, 1, 0.0), (1, 0, 2, -0.5)], {0: -0.25, 1: 0.0}))
    elif name in ("T1", "T2", "T3"):
        arcs = [(0, 1, 1, -0.5), (0, 2, 2, 0.0), (0, 1, 3, -0.25), (1, 2, 4, 0.0), (1, 1, 2, -0.125), (2, 1, 5, 0.0), (2, 2, 1, 0.0),
                (1, 2, 2, -0.5), (2, 0, 3, 0.0)]
        c.update(g=DecodingGraph(3, arcs, {1: 0.0, 2: -0.5}), T=int(name[1:]), B=2)
    elif name == "hlens_0_1_T":
        c.update(g=DecodingGraph(4, random_arcs(rng, 4, 12, 6), {0: -1.0, 1: 0.0, 2: -0.5}), B=3, hlens=[0, 1, 8])
    elif name == "ldv_wider_than_V":
        c.update(g=DecodingGraph(5, random_arcs(rng, 5, 15, 6), random_finals(rng, 5) | {0: -2.0}), B=2, ldv=11)
    elif name == "max_len_2":
        c.update(g=DecodingGraph.from_phrases([[1, 2, 3], [3], [2, 4, 1, 5]], weights=[0.0, -0.5, -0.25], loop=True), max_len=2)
    elif name == "T40":
        c.update(g=DecodingGraph(4, random_arcs(rng, 4, 10, 6), {0: -1.0, 2: 0.0, 3: -0.5}), T=40)
    else:
        raise KeyError(name)
    c.setdefault("hlens", [c["T"]] * c["B"])
    c["max_len"] = c["max_len"] or c["T"]
    c["lp"] = grid(rng, (c["B"], c["T"], c["V"]), -8)
    if name == "empty_path":                                              # all blank is the best labelling
        c["lp"][:, :, 0], c["lp"][:, :, 1:] = -0.125, c["lp"][:, :, 1:] - 1.0
    return c


EXACT = ["Q1_A1", "in_degree_32", "in_degree_33", "in_degree_64", "in_degree_65", "in_degree_2000", "A1023", "A1024", "A1025", "self_loops",
         "parallel_arcs_equal_labels", "same_src_and_label_two_dst", "unreachable_node", "no_reachable_final", "empty_path", "T1", "T2", "T3",
         "hlens_0_1_T", "ldv_wider_than_V", "max_len_2", "T40"]


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("name", EXACT)
def test_exact_mode_equals_the_restatement_bit_for_bit(name, K):
    c = exact_case(name)
    g = c["g"]
    for distinct in MODES:
        want, per = reference(c["lp"], c["hlens"], g, K, distinct, c["max_len"])
        got = Call(c["lp"], c["hlens"], g, K, distinct, c["max_len"], True, ldv=c["ldv"]).run()
        print(f"{name} K={K} {distinct}: Q={g.num_nodes} A={g.num_arcs} n_hyp {want[0].tolist()} score {want[1].tolist()}")
        assert_equal_outputs(got, want)
        if name == "no_reachable_final":
            assert (want[0] == 0).all() and np.isneginf(want[1]).all() and (want[2] == -1).all()
        if name == "hlens_0_1_T":
            assert want[0][0] == 0 and want[0][2] >= 1
        if name == "max_len_2" and K > 1:
            assert (want[2] > 2).any()                                   # a path longer than what is stored
        if name == "empty_path":
            assert want[2][0][0] == 0 and (want[3][0][0] == -1).all()       # the empty path leads: length 0, no arcs
        if name == "parallel_arcs_equal_labels" and K == 8:
            assert want[0][0] == (8 if distinct == "arcs" else 2)         # the graph spells 2 3 and 2 2: tokens mode merges the parallel arcs
        if name.startswith("in_degree_"):
            assert int(np.diff(g.in_ptr).max()) == int(name.split("_")[2])
        if K == 1:                                                        # the dense decode's score and traversal list
            for b, p in enumerate(per):
                ref = R.decode_graph(c["lp"][b], c["hlens"][b], g, np.float32)
                assert np.float32(ref["score"]).tobytes() == p["hyp_score"][0].tobytes()
                if p["n_hyp"]:
                    assert list(p["paths"][0]) == ref["trav_arc"][:ref["n_trav"]].tolist()


@pytest.mark.parametrize("name", ["A_max", "Q_max"])
def test_the_limits(name):
    c = exact_case(name)
    g = c["g"]
    assert (g.num_arcs == MAX_ARCS) if name == "A_max" else (g.num_nodes == MAX_NODES)
    for distinct in MODES:
        want, _ = reference(c["lp"], c["hlens"], g, 2, distinct, c["max_len"])
        got = Call(c["lp"], c["hlens"], g, 2, distinct, c["max_len"], True).run()
        print(f"{name} {distinct}: n_hyp {want[0].tolist()} score {want[1].tolist()}")
        assert_equal_outputs(got, want)
        assert want[0][0] == 2


def dense(logits, hlens, g, normalized):
    """oe_ctc_graph on the same inputs -> score (B), the traversal lists."""
    from openeat_amd import ops
    lg = torch.as_tensor(np.asarray(logits), dtype=torch.float32).to(DEV)
    outs = ops.ctc_graph_decode(lg, torch.as_tensor(np.asarray(hlens)).to(DEV), g, normalized=normalized)
    torch.cuda.synchronize()
    score, n_trav, trav_arc = outs[0].cpu().numpy(), outs[4].cpu().numpy(), outs[5].cpu().numpy()
    return score, [trav_arc[b, :n_trav[b]].tolist() for b in range(len(hlens))]


@pytest.mark.parametrize("name", EXACT)
def test_one_best_equals_oe_ctc_graph_bit_for_bit_on_the_grid(name):
    c = exact_case(name)
    score, trav = dense(c["lp"], c["hlens"], c["g"], True)
    for distinct in MODES:
        n_hyp, hs, hl, ha, _ = Call(c["lp"], c["hlens"], c["g"], 1, distinct, c["max_len"], True).run()
        assert hs[:, 0].tobytes() == score.tobytes(), (hs[:, 0], score)
        for b in range(len(trav)):
            assert n_hyp[b] == int(np.isfinite(score[b]))
            if n_hyp[b]:
                assert hl[b, 0] == len(trav[b]) and ha[b, 0, :min(hl[b, 0], c["max_len"])].tolist() == trav[b][:c["max_len"]]


# ---------------------------------------------------------------- raw mode
RAW_K = 4


@functools.lru_cache(maxsize=None)
def raw_trie():
    """The looped trie of test_ctc_graph_gpu.py's raw-mode test (200 phrases over 40 tokens), rebuilt: logits that speak a few
    of the phrases over noise, T = 120.  The float64 restatement with K + 1 hypotheses: computed once."""
    rng = np.random.default_rng(21)
    V, T = 41, 120
    phrases = list(dict.fromkeys(tuple(int(t) for t in rng.integers(1, V, size=int(rng.integers(2, 5)))) for _ in range(230)))[:200]
    assert len(phrases) == 200
    g = DecodingGraph.from_phrases(phrases, weights=(-rng.random(200)).tolist(), loop=True)
    logits = rng.standard_normal((2, T, V)).astype(np.float32) * 1.5
    for b in range(2):
        t = 3
        while t < T - 30:
            for tok in phrases[int(rng.integers(0, 200))]:
                n = int(rng.integers(1, 4))
                logits[b, t: t + n, tok] += 5.0
                t += n + int(rng.integers(0, 3))
            t += int(rng.integers(2, 10))
    hlens = [T, 97]
    lp64 = [AR.log_softmax(logits[b]) for b in range(2)]
    ref = [N.nbest_graph(lp64[b], hlens[b], g, RAW_K + 1, N.ARCS, np.float64) for b in range(2)]
    return g, logits, hlens, lp64, ref


def test_raw_mode_one_best_equals_oe_ctc_graph_bit_for_bit():
    g, logits, hlens, _, _ = raw_trie()
    score, trav = dense(logits, hlens, g, False)
    assert np.isfinite(score).all()
    for distinct in MODES:
        n_hyp, hs, hl, ha, ht = Call(logits, hlens, g, 1, distinct, logits.shape[1], False).run()
        assert hs[:, 0].tobytes() == score.tobytes(), (hs[:, 0], score)
        for b in range(2):
            assert n_hyp[b] == 1 and ha[b, 0, :hl[b, 0]].tolist() == trav[b] and len(trav[b]) >= 8
            assert ht[b, 0, :hl[b, 0]].tolist() == g.label[trav[b]].tolist()


def frames_of(g, path, lp64, Tb):
    """The best alignment of an arc path as a frame labelling (ctc_graph_ref.decode on its linear chain)."""
    L = len(path)
    fin = np.full(L + 1, -np.inf)
    fin[L] = 0.0
    return R.decode(lp64, Tb, L + 1, np.arange(L), np.arange(1, L + 1), g.label[list(path)], np.zeros(L), fin)["frames"][:Tb]


def test_raw_mode_looped_trie_against_the_float64_restatement():
    g, logits, hlens, lp64, ref = raw_trie()
    T = logits.shape[1]
    n_hyp, hs, hl, ha, ht = Call(logits, hlens, g, RAW_K, "arcs", T, False).run()
    for b in range(2):
        want = ref[b]["hyp_score"]
        assert ref[b]["n_hyp"] == RAW_K + 1 and (want[:-1] - want[1:]).min() >= 1e-3, want      # the reference alone: far enough apart to rank
        assert n_hyp[b] == RAW_K
        paths = [tuple(ha[b, k, :hl[b, k]].tolist()) for k in range(RAW_K)]
        assert len(set(paths)) == RAW_K
        for k, path in enumerate(paths):
            assert g.accepts(frames_of(g, path, lp64[b], hlens[b]).tolist()), (b, k)
            own = N.path_score(lp64[b], hlens[b], path, g.src, g.dst, g.label, g.w, g.final)
            print(f"utterance {b} rank {k}: {len(path)} arcs, device {hs[b, k]:.6f}, its path in float64 {own:.6f}, restatement {want[k]:.6f}")
            np.testing.assert_allclose(hs[b, k], own, rtol=RTOL, atol=ATOL)
            assert ht[b, k, :hl[b, k]].tolist() == g.label[list(path)].tolist()
        assert paths == [tuple(p) for p in ref[b]["paths"][:RAW_K]]
        assert (np.diff(hs[b]) <= 0).all()


def test_two_runs_are_bit_identical():
    g, logits, hlens, _, _ = raw_trie()
    call = Call(logits, hlens, g, 8, "tokens", 16, False)
    first = call.run()
    call.fresh_outputs()
    assert_equal_outputs(call.run(), first)
    assert (first[0] == 8).all()
    alone = Call(logits[1:], hlens[1:], g, 8, "tokens", 16, False).run()          # an output depends on its own utterance only
    assert_equal_outputs(alone, [x[1:] for x in first])


def test_captured_in_a_graph_replays_identically():
    c = exact_case("T3")
    want, _ = reference(c["lp"], c["hlens"], c["g"], 3, "arcs", c["max_len"])
    call = Call(c["lp"], c["hlens"], c["g"], 3, "arcs", c["max_len"], True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.check(call.launch(), "oe_ctc_graph_nbest")
        torch.cuda.synchronize()
        call.fresh_outputs()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            hip.check(call.launch(), "oe_ctc_graph_nbest")
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    seen = []
    for _ in range(2):
        for t in call.out:                                                # fresh sentinels in the buffers the graph writes
            t.fill_(SENT_I if t.dtype == torch.int32 else SENT_F)
        torch.cuda.synchronize()
        assert call.untouched()
        graph.replay()
        torch.cuda.synchronize()
        seen.append(call.numpy())
        assert_equal_outputs(seen[-1], want)
    assert_equal_outputs(seen[0], seen[1])


# ---------------------------------------------------------------- contract
@pytest.mark.parametrize("what,text", [
    ("Q0", b"Q=0"), ("Qbig", b"Q=8065"), ("A0", b"A=0"), ("Abig", b"A=16385"), ("U0", b"U=0"), ("UV", b"U=6"), ("B0", b"B=0"),
    ("T0", b"T=0"), ("Tbig", b"T=1048577"), ("V1", b"V=1"), ("ldv", b"ldv=5"), ("nbest0", b"nbest=0"), ("nbest9", b"nbest=9"),
    ("max_len", b"max_len=0"), ("distinct", b"distinct=2"), ("records", b"records"), ("logits", b"logits"), ("hlens", b"hlens"),
    ("graph", b"graph"), ("workspace", b"workspace"), ("n_hyp", b"output"), ("hyp_score", b"output"), ("hyp_len", b"output"),
    ("hyp_arcs", b"output"), ("hyp_tokens", b"output"), ("in_ptr", b"table"), ("src", b"table"), ("dst", b"table"), ("label", b"table"),
    ("col", b"table"), ("w", b"table"), ("final", b"table"), ("cols", b"table")])
def test_bad_arguments_leave_the_outputs_untouched(what, text):
    c = exact_case("self_loops")
    call = Call(c["lp"], c["hlens"], c["g"], 2, "arcs", 4, True)
    a, g = call.args, call.graph
    if what in ("Q0", "Qbig"):
        g.Q = 0 if what == "Q0" else MAX_NODES + 1
    elif what in ("A0", "Abig"):
        g.A = 0 if what == "A0" else MAX_ARCS + 1
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
    elif what in ("nbest0", "nbest9"):
        a.nbest = 0 if what == "nbest0" else 9
    elif what == "max_len":
        a.max_len = 0
    elif what == "distinct":
        a.distinct = 2
    elif what == "records":
        a.T, g.A = 1 << 20, 2048                                            # T * A * K = 2^32
    elif what == "graph":
        a.graph = None
    elif what in ("logits", "hlens", "workspace", "n_hyp", "hyp_score", "hyp_len", "hyp_arcs", "hyp_tokens"):
        setattr(a, what, None)
    else:
        setattr(g, what, None)
    lib = hip.lib()
    rc = call.launch()
    assert rc != 0 and text in lib.oe_last_error(), lib.oe_last_error()
    torch.cuda.synchronize()
    assert call.untouched()


def test_workspace_bytes_is_zero_outside_the_limits():
    f = hip.lib().oe_ctc_graph_nbest_workspace_bytes
    assert f(2, 10, 3, 5, 9, 4) == workspace_formula(2, 10, 3, 5, 9, 4) > 4 * 2 * 10 * 9 * 4
    assert f(1, 1 << 10, 1, MAX_NODES, MAX_ARCS, 8) == workspace_formula(1, 1 << 10, 1, MAX_NODES, MAX_ARCS, 8)
    for bad in ((0, 10, 3, 5, 9, 4), (2, 0, 3, 5, 9, 4), (2, (1 << 20) + 1, 3, 5, 9, 4), (2, 10, 0, 5, 9, 4), (2, 10, 3, 0, 9, 4),
                (2, 10, 3, MAX_NODES + 1, 9, 4), (2, 10, 3, 5, 0, 4), (2, 10, 3, 5, MAX_ARCS + 1, 4), (-1, 10, 3, 5, 9, 4), (2, 10, 3, 5, 9, 0),
                (2, 10, 3, 5, 9, 9), (1, 1 << 20, 3, 5, 2048, 1), (1, 1 << 17, 3, 5, MAX_ARCS, 1)):
        assert f(*bad) == 0, bad
    assert f(1, (1 << 17) - 1, 3, 5, MAX_ARCS, 1) > 0                        # T * A * K just below 2^31


# ---------------------------------------------------------------- python layers
def test_ops_utterance_groups_equal_the_one_call_result():
    from openeat_amd import ops
    c = exact_case("hlens_0_1_T")
    g = c["g"]
    B, T, V = c["lp"].shape
    lg, hl = torch.from_numpy(c["lp"].astype(np.float32)).to(DEV), torch.tensor(c["hlens"], device=DEV)
    whole = ops.ctc_graph_nbest(lg, hl, g, 3, "tokens", normalized=True)
    per_utt = hip.lib().oe_ctc_graph_nbest_workspace_bytes(1, T, len(g.cols), g.num_nodes, g.num_arcs, 3)
    parts = ops.ctc_graph_nbest(lg, hl, g, 3, "tokens", normalized=True, workspace_cap=per_utt)          # three groups of one
    pairs = ops.ctc_graph_nbest(lg, hl, g, 3, "tokens", normalized=True, workspace_cap=2 * per_utt + 7)  # two and one
    torch.cuda.synchronize()
    want, _ = reference(c["lp"], c["hlens"], g, 3, "tokens", T)
    assert_equal_outputs([t.cpu().numpy() for t in whole], want)
    for name, a, b, d in zip(NAMES, whole, parts, pairs):
        assert a.dtype == b.dtype and torch.equal(a, b) and torch.equal(a, d), name
    with pytest.raises(ValueError, match=str(per_utt)):
        ops.ctc_graph_nbest(lg, hl, g, 3, normalized=True, workspace_cap=per_utt - 1)
    with pytest.raises(TypeError):
        ops.ctc_graph_nbest(lg, hl, [[1, 2]], 3)
    with pytest.raises(ValueError):
        ops.ctc_graph_nbest(lg, hl, g, 9)
    with pytest.raises(ValueError):
        ops.ctc_graph_nbest(lg, hl, g, 2, distinct="words")
    with pytest.raises(ValueError):
        ops.ctc_graph_nbest(lg, hl, DecodingGraph.token_loop(V + 1), 2)      # U = V


@functools.lru_cache(maxsize=None)
def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    model = model.to(DEV).eval()
    i = {k: v.to(DEV) for k, v in g["in"].items()}
    feats, flen = i["feats"][:2], i["flen"][:2]
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        lens = mask.squeeze(1).sum(1).tolist()
        greedy = [AR.collapse(model.ctc.argmax(enc)[b, :lens[b]].cpu().tolist()) for b in range(2)]
    assert all(len(x) >= 2 for x in greedy)
    V = model.vocab_size
    phrases = {tuple(greedy[0]), tuple(greedy[1]), tuple(greedy[0][:-1]), tuple(greedy[0][::-1]), tuple(greedy[1][1:]) or (1,),
               tuple(t % (V - 2) + 1 for t in greedy[0]), (1, 2), (3,)}
    phrases = sorted(phrases)
    graph = DecodingGraph.from_phrases([list(p) for p in phrases], weights=[-0.25 * i for i in range(len(phrases))],
                                       outputs=[f"p{i}" for i in range(len(phrases))])
    return model, feats, flen, graph, lens


def test_model_graph_search_nbest():
    from openeat_amd.utils.decoding_graph import GraphHypothesis
    model, feats, flen, graph, _ = tiny_conformer()
    plain = model.ctc_graph_search(feats, flen, graph)
    res = model.ctc_graph_search(feats, flen, graph, nbest=3)
    toks = model.ctc_graph_search(feats, flen, graph, nbest=3, distinct="tokens")
    for p, r, k in zip(plain, res, toks):
        assert p.nbest is None and p.feasible and r.tokens == p.tokens and r.score == p.score
        assert len(r.nbest) == 3 and all(isinstance(h, GraphHypothesis) for h in r.nbest)
        assert r.nbest[0].tokens == p.tokens and r.nbest[0].score == p.score and r.nbest[0].arcs == [t["arc"] for t in p.traversals]
        assert [h.rank for h in r.nbest] == [0, 1, 2] and r.nbest[0].score >= r.nbest[1].score >= r.nbest[2].score
        assert len({tuple(h.tokens) for h in k.nbest}) == 3 and k.nbest[0].tokens == p.tokens
        assert r.nbest[0].outputs == [o["output"] for o in p.outputs]
    with pytest.raises(ValueError):
        model.ctc_graph_search(feats, flen, graph, nbest=3, beam=10.0)


def test_model_graph_attention_rescoring():
    from openeat_amd.utils.common import add_sos_eos, reverse_pad_list
    model, feats, flen, graph, lens = tiny_conformer()
    one = model.ctc_graph_search(feats, flen, graph)
    first = model.graph_attention_rescoring(feats, flen, graph, nbest=1)
    heavy = model.graph_attention_rescoring(feats, flen, graph, nbest=4, ctc_weight=1e4)
    lists = model.ctc_graph_search(feats, flen, graph, nbest=4, distinct="tokens")
    for b in range(2):
        assert first[b].feasible and first[b].rank == 0 and first[b].tokens == one[b].tokens
        assert heavy[b].rank == 0 and heavy[b].tokens == one[b].tokens
    cw, rw = 0.5, 0.3
    assert model.decoder.r_num_blocks > 0
    mixed = model.graph_attention_rescoring(feats, flen, graph, nbest=4, ctc_weight=cw, reverse_weight=rw)
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        for b in range(2):
            scores = []
            for h in lists[b].nbest:                                        # one decoder call per hypothesis, mixed as asr_model.py:504-528
                ys = torch.tensor([h.tokens], dtype=torch.long, device=DEV)
                yl = torch.tensor([len(h.tokens)], device=DEV)
                ys_in, _ = add_sos_eos(ys, model.sos, model.eos, model.ignore_id)
                r_in, _ = add_sos_eos(reverse_pad_list(ys, yl, model.ignore_id), model.sos, model.eos, model.ignore_id)
                L = ys_in.size(1)
                m = torch.tril(torch.ones(L, L, dtype=torch.bool, device=DEV)).unsqueeze(0)
                l_x, r_x, _ = model.decoder(enc[b: b + 1], mask[b: b + 1], ys_in, r_in, m)
                l_lp, r_lp = torch.log_softmax(l_x[0].double(), -1), torch.log_softmax(r_x[0].double(), -1)
                n = len(h.tokens)
                s = sum(float(l_lp[j, w]) for j, w in enumerate(h.tokens)) + float(l_lp[n, model.eos])
                r = sum(float(r_lp[n - j - 1, w]) for j, w in enumerate(h.tokens)) + float(r_lp[n, model.eos])
                scores.append(s * (1 - rw) + r * rw + h.score * cw)
            order = np.argsort(scores)[::-1]
            print(f"utterance {b}: recomputed {scores}, picked rank {mixed[b].rank} score {mixed[b].score}")
            assert scores[order[0]] - scores[order[1]] > 1e-2               # the recomputed pick is not a near-tie
            assert mixed[b].rank == int(order[0]) and mixed[b].tokens == lists[b].nbest[order[0]].tokens
            np.testing.assert_allclose(mixed[b].score, scores[order[0]], rtol=1e-3, atol=1e-2)


def test_model_an_infeasible_utterance_does_not_disturb_the_others():
    model, feats, flen, _, lens = tiny_conformer()
    n = int(lens[1]) + 1                                                    # n alternating labels need n frames: utterance 1 has n - 1
    assert int(lens[0]) >= n + 1
    chains = [[a if i % 2 == 0 else b for i in range(n)] for a, b in ((1, 2), (2, 1), (1, 3), (3, 4))]
    graph = DecodingGraph.from_phrases(chains, weights=[0.0, -0.25, -0.5, -0.125])
    res = model.graph_attention_rescoring(feats, flen, graph, nbest=3, ctc_weight=0.5, reverse_weight=0.3)
    solo = model.graph_attention_rescoring(feats[:1], flen[:1], graph, nbest=3, ctc_weight=0.5, reverse_weight=0.3)
    assert not res[1].feasible and res[1].rank == -1 and res[1].tokens == [] and np.isneginf(res[1].score)
    assert res[0].feasible and res[0].tokens in chains
    assert res[0].tokens == solo[0].tokens and res[0].rank == solo[0].rank
    np.testing.assert_allclose(res[0].score, solo[0].score, rtol=1e-4, atol=1e-3)
    search = model.ctc_graph_search(feats, flen, graph, nbest=3)
    assert search[0].feasible and len(search[0].nbest) == 3 and not search[1].feasible and search[1].nbest == []
