"""GPU: long-form CTC segmentation (oe_ctc_segment) through the C ABI against the float64 restatement (ctc_segment_ref.py), and
through ops.ctc_segment / ASRModel.ctc_logits_windowed / ASRModel.ctc_segment.

As for the aligner (test_ctc_align_gpu.py): the frame path collapses to the transcript, every move is legal, spans and free
frames are those of the device's own path, `score` is the float64 sum of `path_logp`, and planted paths come back frame for frame.
To the aligner's tolerance (rtol 1e-4 / atol 1e-3) are held `score`, `tok_logp`, `path_logp` and the float64 score of the
device's own path against the float64 optimum; the device's path is never required to EQUAL the float64 path on random logits.

States per thread: the kernel is compiled for 4 / 8 / 16 states per thread, S <= 4096 / 8192 / 16384, and runs ceil(S / NS)
threads rounded up to whole waves, so S = 2 Lmax + 1 crosses a boundary between Lmax = 2047 | 2048 and 4095 | 4096, one wave
becomes two between Lmax = 127 | 128, and Lmax = 8191 fills the last thread of 1024.

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_align_ref as A  # noqa: E402
import ctc_segment_ref as R  # noqa: E402
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def run_seg(logits, hlens, ys, ylens, fs, fe, ldv=None, want=True):
    """-> frames (B, T), path_logp (B, T), start, end, tok_logp (B, Lmax), score (B) as numpy (None what was not asked for)."""
    B, T, V = logits.shape
    ldv = ldv or V
    if ldv == V:
        buf = logits.to(DEV).float().contiguous()
    else:
        buf = torch.zeros(B, T, ldv, device=DEV)
        buf[:, :, :V] = logits.to(DEV)
    Lmax = ys.shape[1]
    hl, yl, yd = hlens.int().to(DEV), ylens.int().to(DEV), ys.int().contiguous().to(DEV)
    L = hip.lib()
    ws = torch.empty(L.oe_ctc_segment_workspace_bytes(B, T, V, Lmax), dtype=torch.uint8, device=DEV)
    frames = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    score = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    pl = st = en = lg = None
    if want:
        pl = torch.full((B, T), float("nan"), device=DEV)
        st = torch.full((B, Lmax), -7, dtype=torch.int32, device=DEV)
        en = torch.full((B, Lmax), -7, dtype=torch.int32, device=DEV)
        lg = torch.full((B, Lmax), float("nan"), device=DEV)
    dp = lambda t: None if t is None else t.data_ptr()
    a = hip.CtcSegmentArgs()
    a.logits, a.ldv, a.B, a.T, a.V = buf.data_ptr(), ldv, B, T, V
    a.hlens, a.targets, a.Lmax, a.tlens = hl.data_ptr(), yd.data_ptr(), Lmax, yl.data_ptr()
    a.free_start, a.free_end = int(fs), int(fe)
    a.frames, a.path_logp, a.tok_start, a.tok_end, a.tok_logp = frames.data_ptr(), dp(pl), dp(st), dp(en), dp(lg)
    a.score, a.workspace = score.data_ptr(), ws.data_ptr()
    hip.check(L.oe_ctc_segment(C.byref(a), hip.stream()), "oe_ctc_segment")
    torch.cuda.synchronize()
    np_ = lambda t: None if t is None else t.cpu().numpy()
    return np_(frames), np_(pl), np_(st), np_(en), np_(lg), np_(score)


def states_of(tokens, ext):
    """The state path of a frame path (unique: a label followed by itself stays, anything else moves on), with the checks
    that it starts and ends where a CTC path may and moves legally."""
    S = len(ext)
    s = 0 if tokens[0] == 0 else 1
    assert s < S and ext[s] == tokens[0], "first frame is neither blank nor the first label"
    states = [s]
    for prev, tok in zip(tokens, tokens[1:]):
        if tok != prev:
            nxt = s + 1 if (tok == 0 or prev == 0) else s + 2
            assert nxt < S and ext[nxt] == tok and A.legal_move(ext, s, nxt), (s, nxt, prev, tok)
            s = nxt
        states.append(s)
    assert s in (S - 1, S - 2), "path does not end in the last label or the last blank"
    return states


def check_recording(b, lp, y, Tb, fs, fe, out, want=None, expect_states=None):
    """One feasible recording's outputs against its log-probabilities lp (Tb, V) float64; want: the float64 optimum."""
    frames, pl, st, en, lg, score = out
    L, ext = len(y), A.ext_labels(y)
    tokens = [int(c) for c in frames[b, :Tb]]
    assert A.collapse(tokens) == y, b
    assert (frames[b, Tb:] == -1).all(), b
    states = states_of(tokens, ext)
    if expect_states is not None:
        diff = [t for t in range(Tb) if states[t] != expect_states[t]]
        assert not diff, (b, len(diff), diff[:5])
    free = R.free_frames(states, L, fs, fe)
    got64 = R.path_score(lp, ext, states, fs, fe)
    if pl is not None:
        assert (pl[b, Tb:] == 0).all() and (pl[b, :Tb][free] == 0).all(), b
        ref_pl = np.where(free, 0.0, lp[np.arange(Tb), np.asarray(ext)[states]])
        np.testing.assert_allclose(pl[b, :Tb], ref_pl, rtol=RTOL, atol=ATOL)
        own = pl[b].astype(np.float64).sum()
        assert abs(score[b] - own) <= 1e-9 * max(abs(own), 1e-300), (b, score[b], own)
    if st is not None:
        s0, e0 = A.spans(states, L)
        assert list(st[b, :L]) == s0 and list(en[b, :L]) == e0, b
        assert (st[b, L:] == -1).all() and (en[b, L:] == -1).all() and (lg[b, L:] == 0).all(), b
        cs = np.concatenate([[0.0], np.cumsum(lp[np.arange(Tb), np.asarray(ext)[states]])])
        ref_lg = [cs[e0[l] + 1] - cs[s0[l]] for l in range(L)]
        np.testing.assert_allclose(lg[b, :L], ref_lg, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(score[b], got64, rtol=RTOL, atol=ATOL)
    if want is not None:
        print(f"rec {b}: Tb={Tb} L={L} flags {int(fs)}{int(fe)} float64 optimum {want:.6f}, device path in float64 {got64:.6f}, "
              f"reported {score[b]:.6f}")
        np.testing.assert_allclose(got64, want, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(score[b], want, rtol=RTOL, atol=ATOL)
    return states


def check_infeasible(b, out):
    frames, pl, st, en, lg, score = out
    assert score[b] == -np.inf and (frames[b] == -1).all(), b
    if pl is not None:
        assert (pl[b] == 0).all() and (st[b] == -1).all() and (en[b] == -1).all() and (lg[b] == 0).all(), b


def check_batch(logits, hl, ys, yl, fs, fe, out):
    """Every recording of a batch against the float64 restatement.  Returns the number of feasible recordings."""
    feasible = 0
    for b in range(logits.shape[0]):
        Tb, L = int(hl[b]), int(yl[b])
        y = [int(c) for c in ys[b, :L]]
        lp = A.log_softmax(logits[b, :Tb].double().numpy())
        want, _ = R.segment(lp, y, fs, fe)
        need = L + sum(1 for i in range(1, L) if y[i] == y[i - 1])
        if Tb == 0 or Tb < need:
            assert want == -np.inf
            check_infeasible(b, out)
            continue
        feasible += 1
        check_recording(b, lp, y, Tb, fs, fe, out, want=want)
    return feasible


SHAPES = [(3, 120, 37, 9, 40), (2, 700, 501, 256, 504), (2, 800, 4233, 300, 4236), (2, 2400, 40, 1100, 40)]


def ragged(B, T, V, Lmax):
    hl = torch.randint(T // 2, T + 1, (B,))
    hl[0] = T
    yl = torch.randint(1, Lmax + 1, (B,))
    yl[-1] = Lmax
    ys = torch.randint(1, V, (B, Lmax))
    ys[0, 1] = ys[0, 0]                                      # one adjacent repeat (a blank must come between)
    yl[0] = max(int(yl[0]), 2)
    return hl, ys, yl


@pytest.mark.parametrize("B,T,V,Lmax,ldv", SHAPES)
def test_random_logits(B, T, V, Lmax, ldv):
    """Lmax of 256 and above is what oe_ctc_align refuses."""
    torch.manual_seed(20 + Lmax)
    logits = torch.randn(B, T, V) * 2
    hl, ys, yl = ragged(B, T, V, Lmax)
    lib = hip.lib()
    if Lmax > 255:
        assert lib.oe_ctc_align_workspace_bytes(B, T, Lmax) > 0          # (it sizes anything; the call refuses)
    feasible = 0
    for fs, fe in FLAGS:
        feasible += check_batch(logits, hl, ys, yl, fs, fe, run_seg(logits, hl, ys, yl, fs, fe, ldv))
    assert feasible >= 4


def planted_batch(seed, B, T, V, Lmax, fs, fe, p_blank=0.5, repeats=True):
    """B planted recordings with ragged lengths -> logits (B, T, V), hl, ys, yl, states per recording."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, T, V), dtype=np.float32)
    hl, yl, ys, states = [], [], np.zeros((B, Lmax), dtype=np.int64), []
    for b in range(B):
        L = Lmax if b == B - 1 else int(rng.integers(max(Lmax // 2, 1), Lmax + 1))
        y = [int(c) for c in rng.integers(1, V // 2, size=L)]
        if L > 1 and b == 0:
            y[1] = y[0]
        Tb = T if b == 0 else int(rng.integers(T - T // 8, T + 1))
        case = R.planted_case(rng, Tb, V, y, fs, fe, junk=np.arange(V // 2, V), p_blank=p_blank)
        assert case is not None
        logits[b, :Tb] = case[0]
        ys[b, :L] = y
        hl.append(Tb), yl.append(L), states.append(case[1])
    return torch.from_numpy(logits), torch.tensor(hl), torch.from_numpy(ys), torch.tensor(yl), states


@pytest.mark.parametrize("fs,fe", FLAGS)
@pytest.mark.parametrize("B,T,V,Lmax,ldv", SHAPES)
def test_planted_paths_come_back_exactly(B, T, V, Lmax, ldv, fs, fe):
    logits, hl, ys, yl, states = planted_batch(30 + Lmax, B, T, V, Lmax, fs, fe, p_blank=0.3)
    out = run_seg(logits, hl, ys, yl, fs, fe, ldv)
    for b in range(B):
        Tb, y = int(hl[b]), [int(c) for c in ys[b, : int(yl[b])]]
        lp = A.log_softmax(logits[b, :Tb].double().numpy())
        want = R.path_score(lp, A.ext_labels(y), states[b], fs, fe)
        check_recording(b, lp, y, Tb, fs, fe, out, want=want, expect_states=states[b])


def big_planted(seed, T, V, y, p_blank, junk):
    rng = np.random.default_rng(seed)
    logits, states = R.planted_case(rng, T, V, y, True, True, junk=junk, p_blank=p_blank)
    return torch.from_numpy(logits)[None], states


def check_big(logits, y, states, out):
    """Against the planted path alone (no reference run): frames, spans, and the planted path's float64 score."""
    frames, pl, st, en, lg, score = out
    T, L, ext = logits.shape[1], len(y), np.asarray(A.ext_labels(y))
    assert np.array_equal(frames[0], ext[np.asarray(states)])
    s0, e0 = A.spans(states, L)
    assert np.array_equal(st[0], s0) and np.array_equal(en[0], e0)
    lp = A.log_softmax(logits[0].double().numpy())
    free = R.free_frames(states, L, True, True)
    on_path = np.where(free, 0.0, lp[np.arange(T), ext[np.asarray(states)]])
    assert (pl[0][free] == 0).all()
    np.testing.assert_allclose(pl[0], on_path, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(score[0], on_path.sum(), rtol=RTOL, atol=ATOL)
    own = pl[0].astype(np.float64).sum()
    assert abs(score[0] - own) <= 1e-9 * abs(own)
    cs = np.concatenate([[0.0], np.cumsum(on_path)])
    np.testing.assert_allclose(lg[0], cs[np.asarray(e0) + 1] - cs[np.asarray(s0)], rtol=RTOL, atol=ATOL)


def test_planted_path_at_the_label_limit():
    """L = 8191: S = 16383 states on 1024 threads of 16.  No adjacent repeats, blanks visited with probability 0.02."""
    rng = np.random.default_rng(40)
    L, T, V = 8191, 8700, 40
    y = [1 + int(c) % 19 for c in np.cumsum(rng.integers(1, 19, size=L))]      # a step of 1 .. 18 mod 19: never the same twice
    assert all(a != b for a, b in zip(y, y[1:])) and max(y) < 20
    logits, states = big_planted(41, T, V, y, 0.02, np.arange(20, 40))
    check_big(logits, y, states, run_seg(logits, torch.tensor([T]), torch.tensor([y]), torch.tensor([L]), True, True))


def test_cell_index_beyond_2_to_31():
    """132 000 frames x 16383 states = 2.16e9 cells: 32-bit cell or bit offsets would wrap."""
    L, T, V = 8191, 132000, 16
    y = [1 + i % 7 for i in range(L)]
    logits, states = big_planted(42, T, V, y, 0.5, np.arange(8, 16))
    assert T * (2 * L + 1) > 2 ** 31
    frames, pl, st, en, lg, score = run_seg(logits, torch.tensor([T]), torch.tensor([y]), torch.tensor([L]), True, True)
    ext = np.asarray(A.ext_labels(y))
    s0, e0 = A.spans(states, L)
    assert np.array_equal(frames[0], ext[np.asarray(states)])
    assert np.array_equal(st[0], s0) and np.array_equal(en[0], e0)
    assert np.isfinite(score[0]) and abs(score[0] - pl[0].astype(np.float64).sum()) <= 1e-9 * abs(score[0])


EDGE_HL = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129]
EDGE_YL = [1, 0, 3, 5, 0, 7, 9, 2, 9, 4, 9, 1]


@pytest.mark.parametrize("V,ldv", [(37, 37), (37, 39), (3246, 3248), (9000, 9000)])
def test_frame_count_edges(V, ldv):
    """Frame counts around the 64-frame tiles of the back-trace, with an empty target (recordings 1, 4) and an infeasible
    one (recording 2: three labels with a repeat in three frames).  Null optional pointers change nothing."""
    torch.manual_seed(50 + V)
    B, T, Lmax = len(EDGE_HL), 129, 9
    logits = torch.randn(B, T, V) * 2
    hl, yl = torch.tensor(EDGE_HL), torch.tensor(EDGE_YL)
    ys = torch.randint(1, V, (B, Lmax))
    ys[2, 1] = ys[2, 0]
    ys[2, 2] = (ys[2, 1] % (V - 1)) + 1
    for fs, fe in FLAGS:
        out = run_seg(logits, hl, ys, yl, fs, fe, ldv)
        assert check_batch(logits, hl, ys, yl, fs, fe, out) == B - 1
        bare = run_seg(logits, hl, ys, yl, fs, fe, ldv, want=False)
        assert np.array_equal(bare[0], out[0]) and np.array_equal(bare[5], out[5])


@pytest.mark.parametrize("Lmax", [127, 128, 2047, 2048, 4095, 4096])
def test_states_per_thread_classes(Lmax):
    """Either side of every boundary the module docstring lists (Lmax = 8191: test_planted_path_at_the_label_limit); the second
    recording is one label shorter than Lmax, i.e. S just below the boundary inside the larger class."""
    B, V = 2, 40
    T = Lmax + Lmax // 3 + 60
    logits, hl, ys, yl, states = planted_batch(60 + Lmax, B, T, V, Lmax, True, True, p_blank=0.1)
    out = run_seg(logits, hl, ys, yl, True, True)
    for b in range(B):
        Tb, y = int(hl[b]), [int(c) for c in ys[b, : int(yl[b])]]
        lp = A.log_softmax(logits[b, :Tb].double().numpy())
        check_recording(b, lp, y, Tb, True, True, out, want=R.path_score(lp, A.ext_labels(y), states[b], True, True),
                        expect_states=states[b])


def test_rows_staged_through_lds_at_a_wide_vocabulary():
    """The kernel gathers the labels' logits either from the logits' rows or, where a workgroup can load a row coalesced with
    at most 8 elements per thread and two rows fit 48 KiB of LDS (V <= 8 x threads and V <= 6144), from rows staged in LDS.
    The cases above take the first route at V >= 3246 and the second with one to three elements per thread; this one stages
    V = 4233 on 1024 threads, five elements per thread with a ragged last one."""
    B, V, Lmax = 1, 4233, 2047
    T = Lmax + Lmax // 3 + 60
    logits, hl, ys, yl, states = planted_batch(65, B, T, V, Lmax, True, True, p_blank=0.1)
    out = run_seg(logits, hl, ys, yl, True, True)
    y = [int(c) for c in ys[0]]
    lp = A.log_softmax(logits[0].double().numpy())
    check_recording(0, lp, y, T, True, True, out, want=R.path_score(lp, A.ext_labels(y), states[0], True, True), expect_states=states[0])


def run_align(logits, hl, ys, yl):
    B, T, V = logits.shape
    Lmax = ys.shape[1]
    buf = logits.to(DEV).float().contiguous()
    hld, yld, yd = hl.int().to(DEV), yl.int().to(DEV), ys.int().contiguous().to(DEV)
    L = hip.lib()
    ws = torch.empty(L.oe_ctc_align_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=DEV)
    frames = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    score = torch.full((B,), float("nan"), device=DEV)
    hip.check(L.oe_ctc_align(hip.ptr(buf), V, B, T, V, hip.ptr(hld), hip.ptr(yd), Lmax, hip.ptr(yld), hip.ptr(frames), None, None, None,
                             hip.ptr(score), hip.ptr(ws), hip.stream()), "oe_ctc_align")
    torch.cuda.synchronize()
    return frames.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("B,T,V,Lmax", [(3, 120, 37, 9), (2, 700, 501, 255)])
def test_agrees_with_the_aligner_without_flags(B, T, V, Lmax):
    logits, hl, ys, yl, states = planted_batch(70 + Lmax, B, T, V, Lmax, False, False, p_blank=0.3)
    seg = run_seg(logits, hl, ys, yl, False, False)
    al_frames, _ = run_align(logits, hl, ys, yl)
    assert np.array_equal(seg[0], al_frames)
    torch.manual_seed(71 + Lmax)
    logits = torch.randn(B, T, V) * 2
    hl, ys, yl = ragged(B, T, V, Lmax)
    seg = run_seg(logits, hl, ys, yl, False, False)
    _, al_score = run_align(logits, hl, ys, yl)
    n = 0
    for b in range(B):
        Tb, y = int(hl[b]), [int(c) for c in ys[b, : int(yl[b])]]
        want, _, _ = A.align(A.log_softmax(logits[b, :Tb].double().numpy()), y)
        if want == -np.inf:
            assert seg[5][b] == -np.inf and al_score[b] == -np.inf
            continue
        n += 1
        np.testing.assert_allclose(seg[5][b], want, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(al_score[b], want, rtol=RTOL, atol=ATOL)
    assert n >= 1


def test_too_many_labels_are_refused_before_any_launch():
    B, T, V, Lmax = 1, 20, 8, 8192
    z = torch.zeros(B, T, V, device=DEV)
    hl = torch.tensor([T], dtype=torch.int32, device=DEV)
    yl = torch.tensor([Lmax], dtype=torch.int32, device=DEV)
    ys = torch.ones(B, Lmax, dtype=torch.int32, device=DEV)
    frames = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    pl = torch.full((B, T), 5.0, device=DEV)
    st = torch.full((B, Lmax), -7, dtype=torch.int32, device=DEV)
    score = torch.full((B,), 3.0, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    lib = hip.lib()
    assert lib.oe_ctc_segment_workspace_bytes(B, T, V, Lmax) == 0
    a = hip.CtcSegmentArgs()
    a.logits, a.ldv, a.B, a.T, a.V = z.data_ptr(), V, B, T, V
    a.hlens, a.targets, a.Lmax, a.tlens = hl.data_ptr(), ys.data_ptr(), Lmax, yl.data_ptr()
    a.free_start, a.free_end = 1, 1
    a.frames, a.path_logp, a.tok_start, a.score, a.workspace = frames.data_ptr(), pl.data_ptr(), st.data_ptr(), score.data_ptr(), ws.data_ptr()
    rc = lib.oe_ctc_segment(C.byref(a), hip.stream())
    assert rc != 0 and b"8191-label limit" in lib.oe_last_error()
    torch.cuda.synchronize()
    assert bool((frames == -7).all()) and bool((pl == 5.0).all()) and bool((st == -7).all()) and float(score[0]) == 3.0


def test_segment_captured_in_a_graph_replays_bit_for_bit():
    from openeat_amd import ops
    torch.manual_seed(80)
    B, T, V, Lmax = 4, 300, 200, 300
    hl = torch.tensor([300, 190, 299, 120], dtype=torch.int32, device=DEV)
    yl = torch.tensor([280, 12, 1, 300], dtype=torch.int32, device=DEV)          # recording 3 infeasible
    ys = torch.randint(1, V, (B, Lmax), dtype=torch.int32, device=DEV)
    static = torch.randn(B, T, V, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ctc_segment(static, V, B, T, V, hl, ys, yl)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = ops.ctc_segment(static, V, B, T, V, hl, ys, yl)
    torch.cuda.current_stream().wait_stream(s)
    for seed in (81, 82):
        fresh = torch.randn(B, T, V, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 2
        static.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.ctc_segment(fresh.clone(), V, B, T, V, hl, ys, yl)
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
        assert float(eager[5][3]) == float("-inf") and torch.isfinite(eager[5][:3]).all()


def test_ops_segment_with_no_label_columns():
    """ys of shape (B, 0): with free_start every valid frame is free; without flags every valid frame is a scored blank."""
    from openeat_amd import ops
    torch.manual_seed(83)
    B, T, V = 2, 40, 30
    logits = torch.randn(B, T, V, device=DEV)
    hl = torch.tensor([40, 17], device=DEV)
    none, zero = torch.zeros(B, 0, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    frames, pl, st, en, lg, score = ops.ctc_segment(logits, V, B, T, V, hl, none, zero)
    assert st.shape == en.shape == lg.shape == (B, 0) and score.dtype == torch.float64
    frames = frames.cpu()
    assert bool((frames[0] == 0).all()) and bool((frames[1, :17] == 0).all()) and bool((frames[1, 17:] == -1).all())
    assert bool((pl == 0).all()) and bool((score == 0).all())
    lp = logits.cpu().double().log_softmax(-1)[:, :, 0]
    _, pl, _, _, _, score = ops.ctc_segment(logits, V, B, T, V, hl, none, zero, free_start=False, free_end=False)
    torch.testing.assert_close(score.cpu(), torch.stack([lp[0].sum(), lp[1, :17].sum()]), rtol=RTOL, atol=ATOL)
    _, pl, _, _, _, score = ops.ctc_segment(logits, V, B, T, V, hl, none, zero, free_start=False, free_end=True)
    torch.testing.assert_close(score.cpu(), lp[:, 0], rtol=RTOL, atol=ATOL)      # frame 0 is scored, the rest is free
    assert bool((pl[:, 1:] == 0).all())


def recording():
    """The tiny conformer and its fixture's utterances concatenated in time into one recording."""
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    feats, flen = g["in"]["feats"], g["in"]["flen"]
    rec = torch.cat([feats[b, : int(flen[b])] for b in range(feats.shape[0])])[None].to(DEV)
    return model.to(DEV).eval(), rec, torch.tensor([rec.shape[1]], device=DEV)


def test_windowed_logits_are_the_windows_own_rows():
    from openeat_amd.utils.segment import encoder_frames, window_plan
    model, rec, n = recording()
    embed = model.encoder.embed
    n_enc = encoder_frames(int(n[0]), embed.subsampling_rate, embed.right_context)
    with torch.no_grad():
        enc, mask, _ = model._encode(rec, n)
        plain = model.ctc.logits(enc)
        assert int(mask.sum()) == n_enc == plain.shape[1]
        whole, lens = model.ctc_logits_windowed(rec, n, n_enc, 4)
        assert torch.equal(whole, plain) and lens.tolist() == [n_enc]
        window, margin = 8, 4
        assert window < n_enc
        got, lens = model.ctc_logits_windowed(rec, n, window, margin)
        assert got.shape == plain.shape and lens.tolist() == [n_enc]
        plan = window_plan(int(n[0]), window, margin, embed.subsampling_rate, embed.right_context)
        assert len(plan) > 2
        flen = torch.tensor([f1 - f0 for f0, f1, _, _, _ in plan], device=DEV)
        batch = torch.zeros(len(plan), int(flen.max()), rec.shape[2], device=DEV)
        for w, (f0, f1, _, _, _) in enumerate(plan):
            batch[w, : f1 - f0] = rec[0, f0:f1]
        mine = model.ctc.logits(model._encode(batch, flen)[0])
        for w, (_, _, q0, q1, o0) in enumerate(plan):
            assert torch.equal(got[0, o0:o0 + q1 - q0], mine[w, q0:q1]), w


def test_model_ctc_segment_end_to_end():
    from openeat_amd import ops
    from openeat_amd.utils.align import frame_times
    from openeat_amd.utils.segment import segment_stats
    model, rec, n = recording()
    with torch.no_grad():
        enc, mask, _ = model._encode(rec, n)
        logits = model.ctc.logits(enc)
        Tp, V = logits.shape[1], logits.shape[2]
        y = A.collapse(model.ctc.argmax(enc)[0].tolist())
    assert len(y) >= 3
    cut = [0, len(y) // 3, 2 * len(y) // 3, len(y)]
    utts = [y[a:b] for a, b in zip(cut, cut[1:])]
    res = model.ctc_segment(rec, n, [utts], with_times=True, score_window=5)
    assert len(res) == 1 and set(res[0]) == {"score", "utterances"} and len(res[0]["utterances"]) == 3
    lens = torch.tensor([Tp], device=DEV)
    ys, yl = torch.tensor([y], device=DEV), torch.tensor([len(y)], device=DEV)
    _, pl, st, en, _, score = ops.ctc_segment(logits, V, 1, Tp, V, lens, ys, yl)
    s, e, mean, mn = (c.cpu().tolist() for c in segment_stats(pl[0], st[0], en[0], cut, 5))
    assert res[0]["score"] == float(score[0]) and np.isfinite(res[0]["score"])
    rate = model.encoder.embed.subsampling_rate
    last = -1
    for u, seg in enumerate(res[0]["utterances"]):
        assert set(seg) == {"start_frame", "end_frame", "mean_logp", "min_logp", "confidence", "start_s", "end_s"}
        assert last < seg["start_frame"] <= seg["end_frame"] < Tp                 # ordered, no overlap
        last = seg["end_frame"]
        assert (seg["start_frame"], seg["end_frame"], seg["mean_logp"], seg["min_logp"]) == (s[u], e[u], mean[u], mn[u])
        assert (seg["start_s"], seg["end_s"]) == frame_times(s[u], e[u], rate)
        assert 0.0 < seg["confidence"] <= 1.0 and seg["confidence"] == pytest.approx(np.exp(mn[u]))
        assert seg["min_logp"] <= seg["mean_logp"] + 1e-12
    plain = model.ctc_segment(rec, n, [utts])
    assert set(plain[0]["utterances"][0]) == {"start_frame", "end_frame", "mean_logp", "min_logp", "confidence"}
    assert model.ctc_segment(rec, n, [[list(range(1, 20)) * 3, [1] * Tp]]) == [None]    # more labels than frames
    win = model.ctc_segment(rec, n, [utts], window=8, margin=4, with_times=True)
    assert len(win) == 1 and set(win[0]) == {"score", "utterances"} and len(win[0]["utterances"]) == 3
    assert all(set(a) == set(b) for a, b in zip(win[0]["utterances"], res[0]["utterances"]))
    with pytest.raises(ValueError):
        model.ctc_segment(rec, n, [[y, []]])
