"""GPU: the row pass of the keyword and graph CTC decoders (lp_rows_kernel, lp_rows.hip) read back directly.

One kernel stands behind oe_ctc_kws, oe_ctc_graph, oe_ctc_graph_logp, oe_ctc_graph_beam and oe_ctc_graph_nbest, whose own raw-mode
tests stay at V <= 50 and so never enter its unrolled main loop (8 x 64 columns a trip).  Here oe_ctc_graph is called with a
graph of one node and a self-loop per wanted label, and the row table is read from the head of the workspace (ctc_graph.hip:
cw = workspace + 0, B * T rows of U + 1 floats: the blank, then the graph's distinct labels ascending).

V = 5 .. 4233 covers the tail-only path and both sides of one and two trips of the main loop and its remainder; U = 70 gives the
gather loop a second trip; labels outside [0, V) must read the nearest column.  B = 3, T = 5, hlens = 5, 1, 0; ldv = V + 3 with
3.0e4 behind V, which a read past V would turn into an infinite log-sum-exp.

Tolerance.  The logits are randn * 3, all finite, |x| <= ~15, so |lp| < 32 and the two float32 roundings of wm + log(s) and
x - c cost < 4e-6; a float32 sum of at most 67 terms per lane and the wave merge have a relative error < 1e-5 in s, the same
absolute error in log(s).  The rows are held to an absolute 1e-4 of float64 x[col] - logsumexp(x[:V]), about five times that.
Rows of frames t >= hlens[b] keep the sentinel the workspace was filled with; with normalized=1 the rows are the gathered
inputs bit for bit; two runs agree in every bit.

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openeat_amd import hip  # noqa: E402
from openeat_amd.utils.decoding_graph import DecodingGraph  # noqa: E402

DEV = "cuda"
B, T, HLENS = 3, 5, (5, 1, 0)
PAD, BEHIND = 3, 3.0e4
SENT = -777.0
ATOL = 1e-4

CASES = {f"V{V}": (V, (1, V // 2, V - 1)) for V in (5, 63, 64, 65, 511, 512, 513, 1025, 4233)}
CASES["V513_U70"] = (513, tuple(range(1, 491, 7)))                          # 70 labels: the gather loop's second trip
CASES["V513_labels_outside"] = (513, (1, 256, 512, 513, 600, -2))           # 513, 600 read column 512; -2 reads the blank


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x (B, T, V) float32, cols (U) int32 ascending, want_raw, want_norm (B, T, U + 1)): float64 lp and the gathered inputs."""
    V, labels = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    cols = np.unique(np.asarray(labels, dtype=np.int32))
    read = np.concatenate([[0], np.clip(cols, 0, V - 1)])                   # the columns a compact row holds
    x64 = x.astype(np.float64)
    m = x64.max(axis=2, keepdims=True)
    lse = m + np.log(np.exp(x64 - m).sum(axis=2, keepdims=True))
    for a in (x, cols):
        a.setflags(write=False)
    return x, cols, x64[:, :, read] - lse, x[:, :, read]


def row_table(name, normalized):
    """The row table oe_ctc_graph leaves at the head of a sentinel-filled workspace, (B, T, U + 1) float32."""
    x, cols, _, _ = case(name)
    V, U = x.shape[2], len(cols)
    g = DecodingGraph(1, [(0, 0, 1, 0.0)] * U, {0: 0.0})
    g.label = cols.copy()                                                   # none is checked: labels outside [0, V) among them
    g.cols = cols.copy()
    g.col = np.arange(U, dtype=np.int32)
    buf = torch.full((B, T, V + PAD), BEHIND, device=DEV)
    buf[:, :, :V] = torch.tensor(x, device=DEV)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in g.host_tables()]
    in_ptr, src, dst, label, col, w, final, cols_d = t
    graph = hip.DecodingGraph(1, U, in_ptr.data_ptr(), src.data_ptr(), dst.data_ptr(), label.data_ptr(), col.data_ptr(), w.data_ptr(),
                              final.data_ptr(), cols_d.data_ptr(), U)
    hl = torch.tensor(HLENS, dtype=torch.int32, device=DEV)
    nbytes = hip.lib().oe_ctc_graph_workspace_bytes(B, T, U, 1, U)
    assert nbytes >= 4 * B * T * (U + 1) and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), SENT, dtype=torch.float32, device=DEV)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)
    out = [torch.empty(B, device=DEV), i32(B, T), i32(B, T), i32(B), i32(B, T), i32(B, T), i32(B, T)]
    a = hip.CtcGraphArgs()
    a.logits, a.ldv, a.B, a.T, a.V, a.hlens = buf.data_ptr(), V + PAD, B, T, V, hl.data_ptr()
    a.graph, a.normalized, a.max_trav, a.workspace = C.pointer(graph), int(normalized), T, ws.data_ptr()
    a.score, a.frames, a.arcs, a.n_trav, a.trav_arc, a.trav_start, a.trav_end = (o.data_ptr() for o in out)
    a.path_logp = a.trav_logp = None
    hip.check(hip.lib().oe_ctc_graph(C.byref(a), hip.stream()), "oe_ctc_graph")
    torch.cuda.synchronize()
    return ws[:B * T * (U + 1)].cpu().numpy().reshape(B, T, U + 1)


def split(rows):
    """-> (the rows of the frames t < hlens[b], the rows behind them), each flattened to (n, U + 1)."""
    live = np.arange(T)[None, :] < np.asarray(HLENS)[:, None]
    return rows[live], rows[~live]


@pytest.mark.parametrize("name", list(CASES))
def test_raw_rows_are_x_minus_logsumexp(name):
    _, cols, want, _ = case(name)
    got = row_table(name, False)
    live, behind = split(got)
    assert np.isfinite(live).all()
    err = float(np.abs(live.astype(np.float64) - split(want)[0]).max())
    print(f"{name}: V={CASES[name][0]} U={len(cols)} max |lp - float64| = {err:.3e}")
    assert err <= ATOL
    assert (behind == np.float32(SENT)).all()
    assert np.array_equal(got, row_table(name, False))                      # a second run: every bit


@pytest.mark.parametrize("name", list(CASES))
def test_normalized_rows_are_the_gathered_inputs(name):
    _, _, _, want = case(name)
    live, behind = split(row_table(name, True))
    assert np.array_equal(live, split(want)[0])
    assert (behind == np.float32(SENT)).all()
