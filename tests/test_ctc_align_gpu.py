"""GPU: CTC forced alignment (oe_ctc_align) through the C ABI against a float64 loop-level restatement (ctc_align_ref.py), and
through CTC.forced_align / ASRModel.ctc_align.

What is held exactly: the frame path collapses to the target, every move is legal, spans are those of the device's own path,
and planted alignments come back frame for frame.  What is held to a tolerance: scores and span log-probs, rtol 1e-4 / atol 1e-3 -
the tolerance the CTC loss is held to against aten (test_ctc_vs_oracle); the device works on float32 base-2 log-probs.  The
device's path is never required to EQUAL the float64 path on random logits (float32 may break a near-tie the other way); it is
required to SCORE like it, which is what optimality means.

The file is not named test_gpu_*: conftest.py orders those files by a fixed list that test_host_logic.py holds complete.  These
are kernel-level proofs; outside the list they are collected in front of it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_align_ref as R  # noqa: E402
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3


def run_align(logits, hlens, ys, ylens, ldv=None, want_tok=True):
    """-> frames (B, T), start, end (B, Lmax), tok_logp (B, Lmax), score (B) as numpy (the tok_* None when not asked for)."""
    B, T, V = logits.shape
    ldv = ldv or V
    buf = torch.zeros(B, T, ldv, device=DEV)
    buf[:, :, :V] = logits.to(DEV)
    Lmax = ys.shape[1]
    hl, yl, yd = hlens.int().to(DEV), ylens.int().to(DEV), ys.int().contiguous().to(DEV)
    L = hip.lib()
    ws = torch.empty(L.oe_ctc_align_workspace_bytes(B, T, Lmax), dtype=torch.uint8, device=DEV)
    frames = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    score = torch.full((B,), float("nan"), device=DEV)
    st = en = lg = None
    if want_tok:
        st = torch.full((B, Lmax), -7, dtype=torch.int32, device=DEV)
        en = torch.full((B, Lmax), -7, dtype=torch.int32, device=DEV)
        lg = torch.full((B, Lmax), float("nan"), device=DEV)
    hip.check(L.oe_ctc_align(hip.ptr(buf), ldv, B, T, V, hip.ptr(hl), hip.ptr(yd), Lmax, hip.ptr(yl), hip.ptr(frames), hip.ptr(st),
                             hip.ptr(en), hip.ptr(lg), hip.ptr(score), hip.ptr(ws), hip.stream()), "oe_ctc_align")
    torch.cuda.synchronize()
    np_ = lambda t: None if t is None else t.cpu().numpy()
    return np_(frames), np_(st), np_(en), np_(lg), np_(score)


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
            assert nxt < S and ext[nxt] == tok and R.legal_move(ext, s, nxt), (s, nxt, prev, tok)
            s = nxt
        states.append(s)
    assert s in (S - 1, S - 2), "path does not end in the last label or the last blank"
    return states


def check_batch(logits, hl, ys, yl, out, expect_states=None):
    """Every utterance of a batch against the float64 restatement.  Returns the number of feasible utterances."""
    frames, st, en, lg, score = out
    B, T, V = logits.shape
    Lmax = ys.shape[1]
    feasible = 0
    for b in range(B):
        Tb, L = int(hl[b]), int(yl[b])
        y = [int(c) for c in ys[b, :L]]
        lp = R.log_softmax(logits[b, :Tb].double().numpy())
        want, ref_states, _ = R.align(lp, y)
        need = L + sum(1 for i in range(1, L) if y[i] == y[i - 1])
        if Tb == 0 or Tb < need:
            assert want == -np.inf
            assert score[b] == -np.inf and (frames[b] == -1).all(), b
            if st is not None:
                assert (st[b] == -1).all() and (en[b] == -1).all() and (lg[b] == 0).all(), b
            continue
        feasible += 1
        ext = R.ext_labels(y)
        tokens = [int(c) for c in frames[b, :Tb]]
        assert R.collapse(tokens) == y, b                                   # (a)
        assert (frames[b, Tb:] == -1).all(), b
        states = states_of(tokens, ext)                                     # (b)
        if st is not None:                                                  # (c) along the device's own path
            s0, e0 = R.spans(states, L)
            assert list(st[b, :L]) == s0 and list(en[b, :L]) == e0, b
            assert (st[b, L:] == -1).all() and (en[b, L:] == -1).all() and (lg[b, L:] == 0).all(), b
            ref_lg = [lp[s0[l]:e0[l] + 1, y[l]].sum() for l in range(L)]
            np.testing.assert_allclose(lg[b, :L], ref_lg, rtol=RTOL, atol=ATOL)
        got64 = R.path_score(lp, ext, states)                               # (d)
        print(f"utt {b}: Tb={Tb} L={L} float64 optimum {want:.6f}, device path in float64 {got64:.6f}, reported {score[b]:.6f}, "
              f"path equals the float64 path: {states == ref_states}")
        np.testing.assert_allclose(got64, want, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(score[b], want, rtol=RTOL, atol=ATOL)
        if expect_states is not None:
            assert states == expect_states[b], b
    return feasible


SHAPES = [(6, 50, 37, 9, 40), (4, 120, 3246, 40, 3248), (3, 90, 501, 70, 504), (2, 300, 100, 140, 100), (2, 400, 4233, 60, 4236)]


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
def test_align_random_logits(B, T, V, Lmax, ldv):
    torch.manual_seed(7)
    logits = torch.randn(B, T, V) * 2
    hl, ys, yl = ragged(B, T, V, Lmax)
    out = run_align(logits, hl, ys, yl, ldv=ldv)
    assert check_batch(logits, hl, ys, yl, out) >= 1


def plant(Tb, y, gen):
    """A random legal state path of Tb frames through the trellis of y (None if Tb is too short)."""
    L = len(y)
    visit = []
    for l in range(L):
        if (l > 0 and y[l] == y[l - 1]) or torch.rand((), generator=gen) < 0.5:
            visit.append(2 * l)
        visit.append(2 * l + 1)
    if L == 0 or torch.rand((), generator=gen) < 0.5:
        visit.append(2 * L)
    if len(visit) > Tb:
        visit = [s for s in visit if s % 2 == 1 or (0 < s < 2 * L and y[s // 2] == y[s // 2 - 1])]
        if len(visit) > Tb:
            return None
    cuts = sorted((torch.randperm(Tb - 1, generator=gen)[: len(visit) - 1] + 1).tolist()) if len(visit) > 1 else []
    bounds = [0] + cuts + [Tb]
    states = []
    for s, a, b in zip(visit, bounds, bounds[1:]):
        states += [s] * (b - a)
    return states


@pytest.mark.parametrize("B,T,V,Lmax,ldv", SHAPES)
def test_align_planted_paths_come_back_exactly(B, T, V, Lmax, ldv):
    """+8 on the planted token of every frame of randn logits: any other legal path differs in at least one frame and loses
    about 8 nats there (the two logits involved differ by N(0, 2) noise), so the planted path is the optimum by a margin no
    float32 rounding reaches, and frames, start and end must be the planted ones exactly."""
    torch.manual_seed(9)
    gen = torch.Generator().manual_seed(10)
    logits = torch.randn(B, T, V)
    hl, ys, yl = ragged(B, T, V, Lmax)
    hl[-1] = T                                               # the utterance with all Lmax labels gets the frames for them
    yl = torch.minimum(yl, hl - 8)                           # every target fits its frames, a few repeats included
    planted = []
    for b in range(B):
        y = [int(c) for c in ys[b, : int(yl[b])]]
        states = plant(int(hl[b]), y, gen)
        assert states is not None
        ext = R.ext_labels(y)
        assert all(R.legal_move(ext, p, q) for p, q in zip(states, states[1:])) and states[0] <= 1 and states[-1] >= 2 * len(y) - 1
        for t, s in enumerate(states):
            logits[b, t, ext[s]] += 8.0
        planted.append(states)
    out = run_align(logits, hl, ys, yl, ldv=ldv)
    assert check_batch(logits, hl, ys, yl, out, expect_states=planted) == B
    frames, st, en = out[0], out[1], out[2]
    for b in range(B):
        L = int(yl[b])
        ext = R.ext_labels([int(c) for c in ys[b, :L]])
        assert [int(c) for c in frames[b, : int(hl[b])]] == [ext[s] for s in planted[b]]
        s0, e0 = R.spans(planted[b], L)
        assert list(st[b, :L]) == s0 and list(en[b, :L]) == e0


# the rows kernel's variants (register-resident rows of 4 / 8 / 16 / 32 float4 per lane, or read twice) and utterance lengths at
# the edges of the recursion's 32-frame prefetch chunks and of the back-trace's 64-frame tiles: the cases of
# test_ctc_row_variants_and_chunk_edges
@pytest.mark.parametrize("V,ldv", [(37, 37), (37, 39), (37, 40), (1500, 1500), (3246, 3246), (3246, 3248), (5000, 5000), (9000, 9000)])
def test_align_row_variants_and_chunk_edges(V, ldv):
    torch.manual_seed(11)
    T, Lmax = 70, 5
    hl = torch.tensor([70, 1, 2, 32, 33, 34, 3, 65, 64])
    yl = torch.tensor([5, 1, 1, 5, 3, 0, 5, 4, 2])          # utterance 6: five labels in three frames -> infeasible; 5: empty target
    B = hl.numel()
    ys = torch.randint(1, V, (B, Lmax))
    ys[0, 1] = ys[0, 0]
    logits = torch.randn(B, T, V) * 2
    out = run_align(logits, hl, ys, yl, ldv=ldv)
    assert check_batch(logits, hl, ys, yl, out) == B - 1
    assert out[4][6] == -np.inf and (out[0][6] == -1).all()
    assert (out[0][5, :34] == 0).all() and (out[0][5, 34:] == -1).all() and np.isfinite(out[4][5])
    bare = run_align(logits, hl, ys, yl, ldv=ldv, want_tok=False)      # NULL tok_* pointers: frames and score only
    assert bare[1] is None and np.array_equal(bare[0], out[0]) and np.array_equal(bare[4], out[4])


@pytest.mark.parametrize("Lmax,CH", [(9, 32), (40, 16), (100, 8), (200, 4)])
def test_align_every_states_per_lane_class(Lmax, CH):
    """Sp = 2 Lmax + 1 in each of the four classes (1 / 2 / 4 / 8 states per lane, prefetch chunks of CH frames)."""
    torch.manual_seed(13)
    V, T = 300, 2 * Lmax + 10
    edge = 1 + (T - 1) // CH * CH                            # the recursion's chunks start at frame 1: a last chunk exactly full
    hl = torch.tensor([T, edge, max(edge - 1, 2), T - 3])
    yl = torch.tensor([Lmax, max(1, min(Lmax, edge // 2 - 1)), 1, Lmax // 2])
    B = hl.numel()
    ys = (torch.arange(Lmax).repeat(B, 1) * 7 + torch.randint(0, 7, (B, 1))) % (V - 1) + 1      # no adjacent repeats ...
    ys[3, 2] = ys[3, 1]                                                                         # ... but this one
    logits = torch.randn(B, T, V) * 2
    out = run_align(logits, hl, ys, yl)
    assert check_batch(logits, hl, ys, yl, out) == B


def test_align_long_batch_keeps_back_pointers_in_the_workspace():
    """T beyond what the block's LDS holds (960 frames at one byte per lane): the back-pointers go through the workspace."""
    torch.manual_seed(14)
    B, T, V, Lmax = 2, 1100, 50, 20
    hl = torch.tensor([1100, 1000])
    yl = torch.tensor([20, 11])
    ys = torch.randint(1, V, (B, Lmax))
    logits = torch.randn(B, T, V) * 2
    lib = hip.lib()
    assert lib.oe_ctc_align_workspace_bytes(B, T, Lmax) >= B * T * (2 * Lmax + 1) * 4 + B * T * 64
    assert lib.oe_ctc_align_workspace_bytes(B, 900, Lmax) < B * 900 * (2 * Lmax + 1) * 4 + 64
    out = run_align(logits, hl, ys, yl)
    assert check_batch(logits, hl, ys, yl, out) == B


def test_align_refuses_more_than_255_labels():
    B, T, V, Lmax = 1, 600, 20, 256
    z = torch.zeros(B, T, V, device=DEV)
    hl = torch.tensor([T], dtype=torch.int32, device=DEV)
    yl = torch.tensor([Lmax], dtype=torch.int32, device=DEV)
    ys = torch.ones(B, Lmax, dtype=torch.int32, device=DEV)
    frames = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    score = torch.full((B,), 3.0, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    lib = hip.lib()
    rc = lib.oe_ctc_align(hip.ptr(z), V, B, T, V, hip.ptr(hl), hip.ptr(ys), Lmax, hip.ptr(yl), hip.ptr(frames), None, None, None,
                          hip.ptr(score), hip.ptr(ws), hip.stream())
    assert rc != 0 and b"255-label limit" in lib.oe_last_error()
    torch.cuda.synchronize()
    assert bool((frames == -7).all()) and float(score[0]) == 3.0          # nothing was launched


def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), {k: v.to(DEV) for k, v in g["in"].items()}


def test_align_to_own_greedy_path_is_the_greedy_path():
    """Aligned to the collapse of its own per-frame argmax (valid frames only), an utterance's best constrained path is the
    unconstrained best: score = sum of the frame maxima, and the path sits on the argmax wherever the runner-up is further away
    than the score tolerance (elsewhere another path stays inside the tolerance, so nothing can be asked)."""
    model, i = tiny_conformer()
    with torch.no_grad():
        enc, mask, _ = model._encode(i["feats"], i["flen"])
        lens = mask.squeeze(1).sum(1)
        best = model.ctc.argmax(enc).cpu()
        lp_all = R.log_softmax(model.ctc.logits(enc).cpu().double().numpy())
        B, T = best.shape
        targets = [R.collapse(best[b, : int(lens[b])].tolist()) for b in range(B)]
        Lmax = max(len(y) for y in targets)
        ys = torch.full((B, Lmax), -1, dtype=torch.int64)
        for b, y in enumerate(targets):
            ys[b, : len(y)] = torch.tensor(y, dtype=torch.int64)
        yl = torch.tensor([len(y) for y in targets], dtype=torch.int32)
        frames, st, en, lg, score = model.ctc.forced_align(enc, lens, ys.to(DEV), yl.to(DEV))
        frames, score = frames.cpu().numpy(), score.cpu().numpy()
    checked = skipped = 0
    for b in range(B):
        Tb = int(lens[b])
        srt = np.sort(lp_all[b, :Tb], axis=1)
        want = srt[:, -1].sum()
        np.testing.assert_allclose(score[b], want, rtol=RTOL, atol=ATOL)                    # (a)
        clear = (srt[:, -1] - srt[:, -2]) > RTOL * abs(want) + ATOL
        assert np.array_equal(frames[b, :Tb][clear], best[b, :Tb].numpy()[clear]), b        # (b)
        assert (frames[b, Tb:] == -1).all()
        checked += int(clear.sum())
        skipped += int((~clear).sum())
    print(f"greedy consistency: {checked} frames compared, {skipped} under the gap ({100.0 * skipped / (checked + skipped):.1f} %)")
    assert skipped <= 0.10 * (checked + skipped)


def test_model_ctc_align_end_to_end():
    from openeat_amd.utils.align import frame_times
    model, i = tiny_conformer()
    feats, flen = i["feats"], i["flen"]
    torch.manual_seed(15)
    B = feats.shape[0]
    tlen = torch.tensor([7, 5, 12], dtype=torch.int32)                  # utterance 2 has 11 encoder frames: infeasible
    tgt = torch.full((B, 12), -1, dtype=torch.int64)
    for b in range(B):
        tgt[b, : int(tlen[b])] = torch.randint(1, 39, (int(tlen[b]),))
    res = model.ctc_align(feats, flen, tgt.to(DEV), tlen.to(DEV), with_times=True)
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        lens = mask.squeeze(1).sum(1).cpu()
        logits = model.ctc.logits(enc).cpu()
    assert int(lens[2]) < 12
    frames, st, en, lg, score = run_align(logits, lens, tgt.clamp(min=0), tlen)
    assert len(res) == B and res[2] is None and score[2] == -np.inf
    rate = model.encoder.embed.subsampling_rate
    assert rate == 4
    for b in range(2):
        r, Tb, L = res[b], int(lens[b]), int(tlen[b])
        assert set(r) == {"frames", "tokens", "score"}
        assert r["frames"] == frames[b, :Tb].tolist() and len(r["frames"]) == Tb
        assert r["score"] == float(score[b])
        assert len(r["tokens"]) == L
        for l, tok in enumerate(r["tokens"]):
            assert set(tok) == {"token", "start_frame", "end_frame", "confidence", "start_s", "end_s"}
            assert (tok["token"], tok["start_frame"], tok["end_frame"]) == (int(tgt[b, l]), int(st[b, l]), int(en[b, l]))
            assert tok["confidence"] == pytest.approx(float(np.exp(lg[b, l] / (en[b, l] - st[b, l] + 1))), rel=1e-6)
            assert 0.0 < tok["confidence"] <= 1.0
            assert (tok["start_s"], tok["end_s"]) == frame_times(tok["start_frame"], tok["end_frame"], 4)
    plain = model.ctc_align(feats, flen, tgt.to(DEV), tlen.to(DEV))
    assert set(plain[0]["tokens"][0]) == {"token", "start_frame", "end_frame", "confidence"}
    check_batch(logits, lens, tgt.clamp(min=0), tlen, (frames, st, en, lg, score))


def test_align_captured_in_a_graph_replays_bit_for_bit():
    from openeat_amd import ops
    torch.manual_seed(16)
    B, T, V, Lmax = 5, 150, 200, 30
    hl = torch.tensor([150, 90, 149, 64, 20], dtype=torch.int32, device=DEV)
    yl = torch.tensor([30, 12, 1, 30, 25], dtype=torch.int32, device=DEV)          # utterance 4 infeasible
    ys = torch.randint(1, V, (B, Lmax), dtype=torch.int32, device=DEV)
    static = torch.randn(B, T, V, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.ctc_align(static, V, B, T, V, hl, ys, yl)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = ops.ctc_align(static, V, B, T, V, hl, ys, yl)
    torch.cuda.current_stream().wait_stream(s)
    for seed in (17, 18):
        fresh = torch.randn(B, T, V, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 2
        static.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.ctc_align(fresh.clone(), V, B, T, V, hl, ys, yl)
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
        assert float(eager[4][4]) == float("-inf") and torch.isfinite(eager[4][:4]).all()


def test_ops_align_with_no_label_columns():
    """ys of shape (B, 0), as CTCHeadFn accepts it: every utterance has an empty target and every valid frame is blank."""
    from openeat_amd import ops
    torch.manual_seed(19)
    B, T, V = 2, 40, 30
    logits = torch.randn(B, T, V, device=DEV)
    hl = torch.tensor([40, 17], device=DEV)
    frames, st, en, lg, score = ops.ctc_align(logits, V, B, T, V, hl, torch.zeros(B, 0, dtype=torch.int64, device=DEV),
                                              torch.zeros(B, dtype=torch.int64, device=DEV))
    assert st.shape == en.shape == lg.shape == (B, 0)
    frames, score = frames.cpu(), score.cpu().double()
    assert bool((frames[0] == 0).all()) and bool((frames[1, :17] == 0).all()) and bool((frames[1, 17:] == -1).all())
    lp = logits.cpu().double().log_softmax(-1)[:, :, 0]
    want = torch.stack([lp[0].sum(), lp[1, :17].sum()])
    torch.testing.assert_close(score, want, rtol=RTOL, atol=ATOL)
