"""GPU: grammar-constrained CTC decoding (oe_ctc_graph) through the C ABI against the restatement (ctc_graph_ref.py), and
through ops.ctc_graph_decode / ASRModel.ctc_graph_search.

Exact mode (normalized=1): log-probabilities, weights and final weights on the 1/8 grid, where every float32 sum is exact
(test_ctc_graph_ref.py shows the restatement's float32 run identical to its float64 run there), so every output must EQUAL the
float64 restatement bit for bit, unused slots and sentinel-prefilled outputs included.  Raw mode (normalized=0): continuous
logits; the device's path, replayed on the host, must be one the graph accepts, and its float64 rescoring is held to the
aligner's tolerance (rtol 1e-4 / atol 1e-3, as test_ctc_align_gpu.py) against the float64 optimum; spans are never compared.

The kernel runs 1024 threads per utterance (A = 1023, 1024, 1025), gives a node of more than 32 incoming arcs to a wave
(in-degree 32, 33, 63, 64, 65, 1500) and loads a thread's first lp one frame ahead (T = 1, 2, 3; hlens = 0 is "one below").

The cross-check against oe_ctc_align uses logits whose log-softmax is exactly on the grid - one column 0 per row, the others
multiples of 1/8 at or below -104, so that the row's log-sum-exp is 0 in float32 however it is taken - and targets the peaks
spell: oe_ctc_align accumulates base-2 logarithms and converts at the end, so only a score whose terms are all 0 can agree with
a natural-log float32 sum in every bit; the frames, the feasibility and the score then must.

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_align_ref as AR  # noqa: E402
import ctc_graph_ref as R  # noqa: E402
from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import MAX_ARCS, MAX_NODES, DecodingGraph  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3
SENT_I, SENT_F = -7, 5.0
NAMES = ("score", "frames", "arcs", "path_logp", "n_trav", "trav_arc", "trav_start", "trav_end", "trav_logp")
FLOATS = ("score", "path_logp", "trav_logp")


def relabel(g, labels):
    """g with the labels replaced as given (none is checked: labels outside [0, V) among them) and cols / col rebuilt."""
    g.label = np.asarray(labels, dtype=np.int32)
    g.cols = np.unique(g.label).astype(np.int32)
    g.col = np.searchsorted(g.cols, g.label).astype(np.int32)
    return g


class Call:
    """One oe_ctc_graph call with its device buffers: sentinel-filled outputs, run() launches on the current stream."""

    def __init__(self, logits, hlens, g, max_trav, normalized, ldv=None, want_logp=True):
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
        nbytes = hip.lib().oe_ctc_graph_workspace_bytes(B, T, len(g.cols), g.num_nodes, g.num_arcs)
        assert 0 < nbytes <= 4 * B * T * (len(g.cols) + 1 + g.num_nodes + g.num_arcs)      # the row table + 4 bytes per state
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.shape, self.max_trav, self.want_logp = (B, T, V), max_trav, want_logp
        a = self.args = hip.CtcGraphArgs()
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = self.buf.data_ptr(), self.ldv, B, T, V, self.hl.data_ptr()
        a.graph, a.normalized, a.max_trav, a.workspace = C.pointer(self.graph), int(normalized), max_trav, self.ws.data_ptr()
        self.fresh_outputs()

    def fresh_outputs(self):
        B, T, _ = self.shape
        M = self.max_trav
        i32 = lambda *s: torch.full(s, SENT_I, dtype=torch.int32, device=DEV)
        f32 = lambda *s: torch.full(s, SENT_F, dtype=torch.float32, device=DEV)
        lg = self.want_logp
        self.out = [f32(B), i32(B, T), i32(B, T), f32(B, T) if lg else None, i32(B), i32(B, M), i32(B, M), i32(B, M), f32(B, M) if lg else None]
        a = self.args
        (a.score, a.frames, a.arcs, a.path_logp, a.n_trav, a.trav_arc, a.trav_start, a.trav_end, a.trav_logp) = (
            None if t is None else t.data_ptr() for t in self.out)

    def launch(self):
        return hip.lib().oe_ctc_graph(C.byref(self.args), hip.stream())

    def run(self):
        hip.check(self.launch(), "oe_ctc_graph")
        torch.cuda.synchronize()
        return self.numpy()

    def numpy(self):
        return [None if t is None else t.cpu().numpy() for t in self.out]

    def untouched(self):
        return all(bool((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all()) for t in self.out if t is not None)


def reference(lp, hlens, g, max_trav):
    """The float64 restatement of a batch, stacked and cast to the device's dtypes (exact on the grid)."""
    per = [R.decode_graph(lp[b], hlens[b], g, np.float64, max_trav) for b in range(len(hlens))]
    return [np.stack([np.asarray(p[name]) for p in per]).astype(np.float32 if name in FLOATS else np.int32) for name in NAMES], per


def assert_equal_outputs(got, want):
    for name, g, w in zip(NAMES, got, want):
        if g is not None:
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
    maximises over the d arcs of another label."""
    arcs = [(int(rng.choice([0, 2, 3, 1] if d > 8 else [0, 2, 3])), 1, int(c), float(w))
            for c, w in zip(rng.integers(1, V, size=d), grid(rng, d, -4))]
    arcs += [(1, int(rng.integers(2, 4)), c, float(grid(rng, 1, -4)[0])) for c in range(1, V)]
    arcs += [(0, int(rng.integers(2, 4)), int(rng.integers(1, V)), 0.0) for _ in range(3)]
    return DecodingGraph(4, arcs, {2: -0.5, 3: 0.0, 1: -1.0})


def exact_case(name):
    """-> dict(lp (B, T, V) float64 on the 1/8 grid, hlens, g, max_trav, ldv, feasible)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    c = dict(B=1, T=40, V=6, max_trav=40, ldv=None, feasible=True)
    if name == "Q1_A1":
        c.update(g=DecodingGraph(1, [(0, 0, 2, -0.5)], {0: -0.25}))
    elif name.startswith("in_degree_"):
        d = int(name.split("_")[2])
        if name.endswith("equal_labels"):                                 # no second best at node 1
            into = [(0, 1, 3, -0.5), (0, 1, 3, -0.25)][:d]
            c.update(g=DecodingGraph(3, into + [(1, 2, 3, 0.0), (1, 2, 4, -0.125)], {2: 0.0, 1: -2.0}))
        else:
            c.update(g=fan_in(rng, d, c["V"]), T=24 if d >= 1000 else 40)
    elif name in ("A1023", "A1024", "A1025"):
        c.update(g=DecodingGraph(40, random_arcs(rng, 40, int(name[1:]), 6), random_finals(rng, 40)), T=16)
    elif name == "A_max":
        c.update(g=DecodingGraph(64, random_arcs(rng, 64, MAX_ARCS, 9), random_finals(rng, 64)), T=8, V=9, max_trav=8)
    elif name == "Q_max":
        c.update(g=DecodingGraph(MAX_NODES, random_arcs(rng, MAX_NODES, 10000, 9, near_start=0.5), random_finals(rng, MAX_NODES)), T=8, V=9,
                 max_trav=8)
    elif name == "self_loops":
        c.update(g=DecodingGraph(2, [(0, 0, 1, -0.125), (0, 0, 2, 0.0), (0, 1, 3, -0.5), (1, 1, 3, 0.0), (1, 1, 1, -0.25), (1, 0, 4, 0.0)],
                                 {1: 0.0, 0: -1.0}))
    elif name == "parallel_arcs_equal_labels":
        c.update(g=DecodingGraph(3, [(0, 1, 2, -1.0), (0, 1, 2, -0.25), (0, 1, 2, -0.25), (1, 2, 3, -0.5), (1, 2, 3, 0.0), (1, 2, 2, 0.0)],
                                 {2: 0.0}))
    elif name == "same_src_and_label_two_dst":
        c.update(g=DecodingGraph(4, [(0, 1, 2, 0.0), (0, 2, 2, 0.0), (1, 3, 3, -0.5), (2, 3, 4, -0.25), (2, 0, 1, 0.0)], {3: 0.0}))
    elif name == "unreachable_node":
        c.update(g=DecodingGraph(5, [(0, 1, 1, 0.0), (1, 2, 2, 0.0), (3, 2, 4, 0.0), (3, 4, 1, 0.0), (4, 3, 2, 0.0), (2, 1, 5, -0.5)],
                                 {2: 0.0, 4: 0.0}))
    elif name == "no_reachable_final":
        c.update(g=DecodingGraph(4, [(0, 1, 1, 0.0), (1, 0, 2, 0.0), (3, 2, 4, 0.0), (2, 2, 1, 0.0)], {2: 0.0, 3: -1.0}), feasible=False)
    elif name == "finals_change_the_winner":
        c.update(g=DecodingGraph(3, [(0, 1, 1, 0.0), (0, 2, 1, 0.0), (1, 1, 2, 0.0), (2, 2, 2, 0.0)], {1: -3.0, 2: -0.125}))
    elif name in ("T1", "T2", "T3"):
        arcs = [(0, 1, 1, -0.5), (0, 2, 2, 0.0), (0, 1, 3, -0.25), (1, 2, 4, 0.0), (1, 1, 2, -0.125), (2, 1, 5, 0.0), (2, 2, 1, 0.0),
                (1, 2, 2, -0.5), (2, 0, 3, 0.0)]
        c.update(g=DecodingGraph(3, arcs, {1: 0.0, 2: -0.5}), T=int(name[1:]), B=2)          # node 0 is not final: a label is emitted
    elif name == "hlens_0_1_T":
        c.update(g=DecodingGraph(4, random_arcs(rng, 4, 12, 6), {0: -1.0, 1: 0.0, 2: -0.5}), B=3, hlens=[0, 1, 40], feasible=None)
    elif name == "B3_ragged":
        c.update(g=DecodingGraph(6, random_arcs(rng, 6, 20, 6), random_finals(rng, 6) | {0: -2.0}), B=3, hlens=[40, 17, 29])
    elif name == "ldv_wider_than_V":
        c.update(g=DecodingGraph(5, random_arcs(rng, 5, 15, 6), random_finals(rng, 5) | {0: -2.0}), B=2, ldv=11)
    elif name == "labels_outside_the_vocabulary":
        g = DecodingGraph(4, random_arcs(rng, 4, 14, 5), {0: -2.0, 1: 0.0, 3: -0.5})
        lab = g.label.copy()
        lab[[1, 4, 6, 9, 12]] = [15, -2, 17, 15, 12]                       # V = 12: 12, 15, 17 read column 11, -2 reads the blank
        c.update(g=relabel(g, lab), V=12)                                   # at most 4 + 4 distinct labels: U < V
    elif name == "max_trav_1":
        c.update(g=DecodingGraph.from_phrases([[1, 2], [3], [2, 4, 1]], weights=[0.0, -0.5, -0.25], loop=True), max_trav=1)
    elif name == "T5000":
        c.update(g=DecodingGraph(4, random_arcs(rng, 4, 10, 6), {0: -1.0, 2: 0.0, 3: -0.5}), T=5000, max_trav=16)
    else:
        raise KeyError(name)
    c.setdefault("hlens", [c["T"]] * c["B"])
    c["lp"] = grid(rng, (c["B"], c["T"], c["V"]), -8)
    return c


EXACT = ["Q1_A1", "in_degree_1_equal_labels", "in_degree_2_equal_labels", "in_degree_32", "in_degree_33", "in_degree_63", "in_degree_64",
         "in_degree_65", "in_degree_1500", "A1023", "A1024", "A1025", "A_max", "Q_max", "self_loops", "parallel_arcs_equal_labels",
         "same_src_and_label_two_dst", "unreachable_node", "no_reachable_final", "finals_change_the_winner", "T1", "T2", "T3",
         "hlens_0_1_T", "B3_ragged", "ldv_wider_than_V", "labels_outside_the_vocabulary", "max_trav_1", "T5000"]


@pytest.mark.parametrize("name", EXACT)
def test_exact_mode_equals_the_restatement_bit_for_bit(name):
    c = exact_case(name)
    g = c["g"]
    want, per = reference(c["lp"], c["hlens"], g, c["max_trav"])
    got = Call(c["lp"], c["hlens"], g, c["max_trav"], True, ldv=c["ldv"]).run()
    print(f"{name}: Q={g.num_nodes} A={g.num_arcs} U={len(g.cols)} score {want[0].tolist()} n_trav {want[4].tolist()}")
    assert_equal_outputs(got, want)
    if c["feasible"] is not None:
        assert bool(np.isfinite(want[0]).all()) == c["feasible"]
    if name == "max_trav_1":
        assert (want[4] > 1).all()                                      # the count exceeds the stored traversals
    if name == "hlens_0_1_T":
        assert np.isneginf(want[0][0]) and (want[1][0] == -1).all() and np.isfinite(want[0][2])
    if name == "finals_change_the_winner":
        used = set(want[2][0][want[2][0] >= 0].tolist())                 # arcs 0, 1 lead to node 1 and arcs 2, 3 to node 2
        assert used and used <= {2, 3}
        assert per[0]["r_state"][0] == per[0]["r_state"][2] and per[0]["n_state"][1] == per[0]["n_state"][2]   # the final weight decides
    if name.startswith("in_degree_") and not name.endswith("equal_labels"):
        assert int(np.diff(g.in_ptr).max()) == int(name.split("_")[2])
    # the optional outputs are optional: without them the rest is the same
    bare = Call(c["lp"], c["hlens"], g, c["max_trav"], True, ldv=c["ldv"], want_logp=False).run()
    assert bare[3] is None and bare[8] is None
    assert_equal_outputs(bare, want)


def test_two_runs_are_bit_identical():
    c = exact_case("in_degree_65")
    rng = np.random.default_rng(2)
    logits = rng.standard_normal((2, 40, 6)).astype(np.float32) * 3
    call = Call(logits, [40, 31], c["g"], 40, False)
    first = call.run()
    call.fresh_outputs()
    assert_equal_outputs(call.run(), first)
    assert np.isfinite(first[0]).all()


# ---------------------------------------------------------------- raw mode
def replay(g, lp64, Tb, frames, arcs, n_trav, trav_arc, trav_start, trav_end):
    """The device's path on the host: it must be a path of the graph under the CTC topology, and its traversal list must be
    what its arcs say -> its float64 score (lp along it, the weights of the arcs it enters, the final weight)."""
    assert (frames[Tb:] == -1).all() and (arcs[Tb:] == -1).all()
    assert g.accepts(frames[:Tb].tolist())
    node, prev, total, trav = 0, -1, 0.0, []
    for t in range(Tb):
        a = int(arcs[t])
        if a < 0:
            assert frames[t] == 0
            if prev >= 0:
                node = int(g.dst[prev])
        else:
            assert frames[t] == g.label[a]
            if a != prev:
                if prev >= 0:                                            # arc to arc: through the node between, labels differ
                    node = int(g.dst[prev])
                    assert g.label[prev] != g.label[a]
                assert int(g.src[a]) == node, (t, a)
                total += float(g.w[a])
                trav.append([a, t, t])
            else:
                trav[-1][2] = t
        total += lp64[t, int(frames[t])]
        prev = a
    if prev >= 0:
        node = int(g.dst[prev])
    assert np.isfinite(g.final[node])
    assert n_trav == len(trav)
    m = min(len(trav), len(trav_arc))
    assert [list(x) for x in zip(trav_arc[:m].tolist(), trav_start[:m].tolist(), trav_end[:m].tolist())] == trav[:m]
    return total + float(g.final[node])


@functools.lru_cache(maxsize=None)
def raw_trie():
    """A looped trie of 200 phrases over 40 tokens, T = 300: logits that speak a few of the phrases over noise, the float64
    optimum: computed once."""
    rng = np.random.default_rng(21)
    V, T = 41, 300
    phrases = list(dict.fromkeys(tuple(int(t) for t in rng.integers(1, V, size=int(rng.integers(2, 5)))) for _ in range(230)))[:200]
    assert len(phrases) == 200
    g = DecodingGraph.from_phrases(phrases, weights=(-rng.random(200)).tolist(), loop=True)
    logits = rng.standard_normal((1, T, V)).astype(np.float32) * 1.5
    t = 3
    while t < T - 30:
        for tok in phrases[int(rng.integers(0, 200))]:
            n = int(rng.integers(1, 4))
            logits[0, t: t + n, tok] += 5.0
            t += n + int(rng.integers(0, 3))
        t += int(rng.integers(2, 10))
    lp64 = AR.log_softmax(logits[0])
    return g, logits, lp64, R.decode_graph(lp64, T, g)


def test_raw_mode_looped_trie_against_the_float64_optimum():
    g, logits, lp64, ref = raw_trie()
    T = logits.shape[1]
    score, frames, arcs, path_logp, n_trav, ta, ts, te, tl = Call(logits, [T], g, T, False).run()
    mine = replay(g, lp64, T, frames[0], arcs[0], int(n_trav[0]), ta[0], ts[0], te[0])
    print(f"looped trie: Q={g.num_nodes} A={g.num_arcs}, optimum {ref['score']:.6f}, device {score[0]:.6f}, its path rescored {mine:.6f}, "
          f"{int(n_trav[0])} traversals")
    np.testing.assert_allclose(mine, ref["score"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(score[0], ref["score"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(path_logp[0], lp64[np.arange(T), frames[0]], rtol=RTOL, atol=ATOL)
    assert int(n_trav[0]) >= 20 and (ta[0, int(n_trav[0]):] == -1).all() and (tl[0, int(n_trav[0]):] == 0).all()


def test_raw_mode_token_loop_is_the_greedy_decode():
    from openeat_amd import ops
    rng = np.random.default_rng(22)
    B, T, V = 2, 120, 50
    logits = rng.standard_normal((B, T, V)).astype(np.float32) * 3
    hlens = [120, 77]
    srt = np.sort(logits, axis=2)
    assert (srt[:, :, -1] - srt[:, :, -2]).min() > 1e-4                     # no ties
    g = DecodingGraph.token_loop(V)
    score, frames, arcs, _, n_trav, ta, _, _, _ = Call(logits, hlens, g, T, False).run()
    lg = torch.from_numpy(logits).to(DEV)
    toks, lens = ops.ctc_greedy(lg, V, B, T, V, torch.tensor(hlens, device=DEV), 0)      # frames behind hlens count as blank
    toks, lens = toks.cpu().numpy(), lens.cpu().numpy()
    for b in range(B):
        Tb = hlens[b]
        assert frames[b, :Tb].tolist() == logits[b, :Tb].argmax(axis=1).tolist()
        mine = g.label[ta[b, : n_trav[b]]].tolist()
        assert mine == AR.collapse(frames[b, :Tb]) == toks[b, : lens[b]].tolist()
        np.testing.assert_allclose(score[b], AR.log_softmax(logits[b, :Tb]).max(axis=1).sum(), rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------- against oe_ctc_align
def test_linear_chain_equals_oe_ctc_align_bit_for_bit():
    rng = np.random.default_rng(23)
    B, T, V = 4, 60, 7
    hlens = [60, 41, 60, 5]
    logits = -104.0 - rng.integers(0, 64, size=(B, T, V)).astype(np.float64) / 8
    peaks = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        t = 0
        while t < T:                                                        # runs of one column, blanks and repeats among them
            n, col = int(rng.integers(1, 5)), int(rng.integers(0, V)) if rng.random() < 0.7 else 0
            peaks[b, t: t + n] = col
            t += n
    np.put_along_axis(logits, peaks[:, :, None], 0.0, axis=2)
    targets = [AR.collapse(peaks[b, : hlens[b]]) for b in range(B)]
    targets[3] = [1, 1, 1, 1]                                               # 4 labels + 3 repeats in 5 frames: infeasible
    Lmax = max(len(y) for y in targets)
    ys = np.zeros((B, Lmax), dtype=np.int32)
    for b, y in enumerate(targets):
        ys[b, : len(y)] = y
    lg = torch.from_numpy(logits.astype(np.float32)).to(DEV)
    al_frames = torch.full((B, T), SENT_I, dtype=torch.int32, device=DEV)
    al_score = torch.full((B,), SENT_F, dtype=torch.float32, device=DEV)
    ws = torch.empty(hip.lib().oe_ctc_align_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=DEV)
    hip.call("oe_ctc_align", lg, V, B, T, V, torch.tensor(hlens, dtype=torch.int32, device=DEV), torch.from_numpy(ys).to(DEV), Lmax,
             torch.tensor([len(y) for y in targets], dtype=torch.int32, device=DEV), al_frames, None, None, None, al_score, ws)
    torch.cuda.synchronize()
    al_frames, al_score = al_frames.cpu().numpy(), al_score.cpu().numpy()
    for b, y in enumerate(targets):
        score, frames = Call(logits[b: b + 1], hlens[b: b + 1], DecodingGraph.linear(y), T, False).run()[:2]
        assert np.array_equal(frames[0], al_frames[b]), b
        assert score[0].tobytes() == al_score[b].tobytes(), (b, score[0], al_score[b])
        if b < 3:
            assert score[0] == 0.0 and frames[0, : hlens[b]].tolist() == peaks[b, : hlens[b]].tolist() and len(y) >= 5
        else:
            assert np.isneginf(score[0]) and (frames[0] == -1).all()


# ---------------------------------------------------------------- contract
@pytest.mark.parametrize("what,text", [
    ("Q0", b"Q=0"), ("Qbig", b"Q=8065"), ("A0", b"A=0"), ("Abig", b"A=16385"), ("U0", b"U=0"), ("UV", b"U=6"), ("B0", b"B=0"),
    ("T0", b"T=0"), ("Tbig", b"T=1048577"), ("V1", b"V=1"), ("ldv", b"ldv=5"), ("max_trav", b"max_trav=0"), ("logits", b"logits"),
    ("hlens", b"hlens"), ("graph", b"graph"), ("workspace", b"workspace"), ("score", b"output"), ("frames", b"output"), ("arcs", b"output"),
    ("n_trav", b"output"), ("trav_arc", b"output"), ("trav_start", b"output"), ("trav_end", b"output"), ("in_ptr", b"table"),
    ("src", b"table"), ("dst", b"table"), ("label", b"table"), ("col", b"table"), ("w", b"table"), ("final", b"table"), ("cols", b"table")])
def test_bad_arguments_leave_the_outputs_untouched(what, text):
    c = exact_case("self_loops")
    call = Call(c["lp"], c["hlens"], c["g"], 4, True)
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
    elif what == "max_trav":
        a.max_trav = 0
    elif what == "graph":
        a.graph = None
    elif what in ("logits", "hlens", "workspace", "score", "frames", "arcs", "n_trav", "trav_arc", "trav_start", "trav_end"):
        setattr(a, what, None)
    else:
        setattr(g, what, None)
    lib = hip.lib()
    rc = call.launch()
    assert rc != 0 and text in lib.oe_last_error(), lib.oe_last_error()
    torch.cuda.synchronize()
    assert call.untouched()


def test_workspace_bytes_is_zero_outside_the_limits():
    f = hip.lib().oe_ctc_graph_workspace_bytes
    assert f(2, 10, 3, 5, 9) == 4 * 2 * 10 * (3 + 1 + 5 + 3)
    assert f(1, 1 << 20, 1, MAX_NODES, MAX_ARCS) == 4 * (1 << 20) * (2 + MAX_NODES + MAX_ARCS // 4)
    for bad in ((0, 10, 3, 5, 9), (2, 0, 3, 5, 9), (2, (1 << 20) + 1, 3, 5, 9), (2, 10, 0, 5, 9), (2, 10, 3, 0, 9), (2, 10, 3, MAX_NODES + 1, 9),
                (2, 10, 3, 5, 0), (2, 10, 3, 5, MAX_ARCS + 1), (-1, 10, 3, 5, 9)):
        assert f(*bad) == 0, bad
    assert MAX_NODES >= 4096 and MAX_ARCS >= 16384


def test_captured_in_a_graph_replays_identically():
    c = exact_case("B3_ragged")
    want, _ = reference(c["lp"], c["hlens"], c["g"], c["max_trav"])
    call = Call(c["lp"], c["hlens"], c["g"], c["max_trav"], True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.check(call.launch(), "oe_ctc_graph")
        torch.cuda.synchronize()
        call.fresh_outputs()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            hip.check(call.launch(), "oe_ctc_graph")
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


# ---------------------------------------------------------------- python layers
def test_ops_utterance_groups_equal_the_one_call_result():
    from openeat_amd import ops
    c = exact_case("B3_ragged")
    g = c["g"]
    B, T, V = c["lp"].shape
    lg, hl = torch.from_numpy(c["lp"].astype(np.float32)).to(DEV), torch.tensor(c["hlens"], device=DEV)
    whole = ops.ctc_graph_decode(lg, hl, g, normalized=True)
    per_utt = hip.lib().oe_ctc_graph_workspace_bytes(1, T, len(g.cols), g.num_nodes, g.num_arcs)
    parts = ops.ctc_graph_decode(lg, hl, g, normalized=True, workspace_cap=per_utt)          # three groups of one
    pairs = ops.ctc_graph_decode(lg, hl, g, normalized=True, workspace_cap=2 * per_utt + 7)  # two and one
    torch.cuda.synchronize()
    want, _ = reference(c["lp"], c["hlens"], g, T)
    assert_equal_outputs([t.cpu().numpy() for t in whole], want)
    for name, a, b, d in zip(NAMES, whole, parts, pairs):
        assert a.dtype == b.dtype and torch.equal(a, b) and torch.equal(a, d), name
    with pytest.raises(TypeError):
        ops.ctc_graph_decode(lg, hl, [[1, 2]])
    with pytest.raises(ValueError):
        ops.ctc_graph_decode(lg, hl, DecodingGraph.linear([]))             # a graph without arcs has no device form
    with pytest.raises(ValueError):
        ops.ctc_graph_decode(lg, hl, DecodingGraph.token_loop(V + 1))      # U = V


def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), {k: v.to(DEV) for k, v in g["in"].items()}


def test_model_graph_search():
    from openeat_amd.utils.align import frame_times
    from openeat_amd.utils.decoding_graph import GraphResult
    model, i = tiny_conformer()
    feats, flen = i["feats"][:1], i["flen"][:1]
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        Tb = int(mask.squeeze(1).sum(1)[0])
        greedy = AR.collapse(model.ctc.argmax(enc)[0, :Tb].cpu().tolist())
    assert len(greedy) >= 2
    res = model.ctc_graph_search(feats, flen, DecodingGraph.linear(greedy), with_times=True)
    assert len(res) == 1 and isinstance(res[0], GraphResult) and res[0].feasible and res[0].tokens == greedy
    rate = model.encoder.embed.subsampling_rate
    for tr in res[0].traversals:
        assert (tr["start_s"], tr["end_s"]) == frame_times(tr["start_frame"], tr["end_frame"], rate)
        assert 0.0 < tr["confidence"] <= 1.0
    other = [t % (model.vocab_size - 1) + 1 for t in greedy[::-1]] + [1]
    phrases = [greedy, other]
    assert tuple(phrases[0]) != tuple(phrases[1])
    two = model.ctc_graph_search(feats, flen, DecodingGraph.from_phrases(phrases, outputs=["first", "second"]))[0]
    assert two.feasible and two.tokens in phrases and np.isfinite(two.score)
    assert [o["output"] for o in two.outputs] == [["first", "second"][phrases.index(two.tokens)]]
    last = -1
    for tr in two.traversals:                                             # the spans tile the frames in order
        assert last < tr["start_frame"] <= tr["end_frame"] < Tb
        last = tr["end_frame"]
    assert two.outputs[0]["start_frame"] == two.traversals[0]["start_frame"] and two.outputs[0]["end_frame"] == two.traversals[-1]["end_frame"]
    whole = model.ctc_graph_search(feats, flen, DecodingGraph.linear(greedy), window=Tb, margin=4)
    assert whole[0].tokens == greedy
    with pytest.raises(ValueError):
        model.ctc_graph_search(feats, flen, [greedy])
