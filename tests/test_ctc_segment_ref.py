"""CPU: the float64 restatement of long-form CTC segmentation (ctc_segment_ref.py) against brute-force enumeration and against
the alignment restatement; the window plan and the segment statistics of openeat_amd/utils/segment.py; and what oe_ctc_segment
refuses and how much workspace it asks for, through the loaded library (no device is touched: every call here returns before
any launch)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ctc_align_ref as A
import ctc_segment_ref as R
from openeat_amd.utils.segment import encoder_frames, segment_stats, window_plan

FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def brute(lp, y, fs, fe):
    """Every legal state path, scored by path_score: (best score, paths tried)."""
    Tb, ext = lp.shape[0], A.ext_labels(y)
    S = len(ext)
    best, n = -np.inf, 0
    for states in itertools.product(range(S), repeat=Tb):
        if states[0] > 1 or states[-1] < S - 2:
            continue
        if any(not A.legal_move(ext, a, b) for a, b in zip(states, states[1:])):
            continue
        n += 1
        best = max(best, R.path_score(lp, ext, states, fs, fe))
    return best, n


def test_restatement_against_brute_force():
    rng = np.random.default_rng(1)
    cases = 0
    for L in range(3):
        for Tb in range(1, 6):
            for rep in range(4):
                y = [int(c) for c in rng.integers(1, 4, size=L)]
                if rep == 0 and L == 2:
                    y[1] = y[0]                                           # an adjacent repeat
                lp = A.log_softmax(rng.standard_normal((Tb, 4)))
                for fs, fe in FLAGS:
                    want, n = brute(lp, y, fs, fe)
                    got, states = R.segment(lp, y, fs, fe)
                    cases += 1
                    if n == 0:
                        assert got == -np.inf and states is None
                        continue
                    assert got == pytest.approx(want, abs=1e-9), (y, Tb, fs, fe)
                    assert R.path_score(lp, A.ext_labels(y), states, fs, fe) == pytest.approx(got, abs=1e-9)
    assert cases == 240


def test_without_flags_it_is_the_alignment():
    rng = np.random.default_rng(2)
    for T, L in [(1, 0), (5, 0), (9, 3), (40, 12), (25, 20), (6, 9)]:
        y = [int(c) for c in rng.integers(1, 6, size=L)]
        lp = A.log_softmax(rng.standard_normal((T, 7)))
        want, states, _ = A.align(lp, y)
        got, mine = R.segment(lp, y, False, False)
        assert mine == states
        assert (got == want == -np.inf) if states is None else got == pytest.approx(want, abs=1e-9)


@pytest.mark.parametrize("T,V,L", [(60, 12, 9), (400, 40, 60), (800, 4233, 300)])
@pytest.mark.parametrize("fs,fe", FLAGS)
def test_planted_cases_are_their_own_optimum(T, V, L, fs, fe):
    """The generator the GPU tests share: the planted path is what the restatement returns."""
    rng = np.random.default_rng(3)
    y = [int(c) for c in rng.integers(1, V // 2, size=L)]
    y[1] = y[0]
    logits, states = R.planted_case(rng, T, V, y, fs, fe, junk=np.arange(V // 2, V))
    got, mine = R.segment(A.log_softmax(logits), y, fs, fe)
    assert mine == states


def own_length(n, rate):
    """The subsampling modules' own length formulas (modules/subsampling.py)."""
    return {4: ((n - 1) // 2 - 1) // 2, 6: ((n - 1) // 2 - 2) // 3, 8: (((n - 1) // 2 - 1) // 2 - 1) // 2, 1: n}[rate]


@pytest.mark.parametrize("rate,rc", [(4, 6), (6, 14), (8, 14), (1, 0)])
@pytest.mark.parametrize("n_feat", [7, 8, 1000, 1003, 6000])
def test_window_plan_tiles_the_recording(rate, rc, n_feat):
    n_enc = encoder_frames(n_feat, rate, rc)
    if n_enc < 1:
        with pytest.raises(ValueError):
            window_plan(n_feat, 10, 2, rate, rc)
        return
    for window, margin in [(1, 0), (7, 3), (50, 16), (64, 0), (100, 200), (n_enc, 16), (n_enc + 5, 4)]:
        plan = window_plan(n_feat, window, margin, rate, rc)
        at = 0
        for f0, f1, q0, q1, o0 in plan:
            assert o0 == at and q1 > q0 and q1 - q0 <= window             # no gap, no overlap
            at += q1 - q0
            assert 0 <= f0 < f1 <= n_feat
            c0, c1 = o0 - q0, o0 - q0 + own_length(f1 - f0, rate)
            assert c0 == f0 // rate and f0 % rate == 0
            assert c0 == max(0, o0 - margin) and c1 == min(n_enc, o0 + (q1 - q0) + margin)
            assert 0 <= q0 and q1 <= c1 - c0
        assert at == n_enc
        if window >= n_enc:
            assert plan == [(0, rate * (n_enc - 1) + rc + 1, 0, n_enc, 0)]
    assert n_enc <= own_length(n_feat, rate) <= n_enc + (1 if rate == 6 else 0)


def test_window_plan_refuses_bad_arguments():
    for args in [(1000, 0, 4, 4, 6), (1000, 10, -1, 4, 6), (6, 10, 2, 4, 6), (14, 10, 2, 8, 14)]:
        with pytest.raises(ValueError):
            window_plan(*args)


def stats_loop(plp, st, en, offsets, win):
    out = []
    for u in range(len(offsets) - 1):
        s, e = int(st[offsets[u]]), int(en[offsets[u + 1] - 1])
        vals = [float(plp[t]) for t in range(s, e + 1)]
        blocks = [vals[i:i + win] for i in range(0, len(vals), win)]
        out.append((s, e, sum(vals) / len(vals), min(sum(b) / len(b) for b in blocks)))
    return out


@pytest.mark.parametrize("win", [1, 4, 30])
def test_segment_stats_against_a_loop(win):
    g = torch.Generator().manual_seed(4 + win)
    T, L = 211, 23
    plp = -torch.rand(T, generator=g) * 5
    cuts = torch.sort(torch.randperm(T - 10, generator=g)[: 2 * L]).values + 5
    st, en = cuts[0::2].int(), cuts[1::2].int()
    offsets = [0, 1, 4, 5, 17, 23]
    got = segment_stats(plp, st, en, offsets, win)
    want = stats_loop(plp.double(), st, en, offsets, win)
    assert got[0].tolist() == [w[0] for w in want] and got[1].tolist() == [w[1] for w in want]
    lens = [w[1] - w[0] + 1 for w in want]
    assert any(n % win for n in lens) or win == 1                         # partial last blocks occur
    np.testing.assert_allclose(got[2].numpy(), [w[2] for w in want], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got[3].numpy(), [w[3] for w in want], rtol=1e-12, atol=1e-12)
    assert got[2].dtype == got[3].dtype == torch.float64


def test_segment_stats_refuses_bad_offsets():
    plp, st, en = torch.zeros(10), torch.tensor([1, 3, 5]), torch.tensor([2, 4, 6])
    for offsets in ([0, 1, 1, 3], [1, 3], [0, 2], [0, 3, 2], [0]):
        with pytest.raises(ValueError):
            segment_stats(plp, st, en, offsets)
    with pytest.raises(ValueError):
        segment_stats(plp, st, en, [0, 3], win=0)


def seg_args(**kw):
    """Arguments that would pass, over fake non-null pointers: every call made with them returns before it launches."""
    from openeat_amd import hip
    a = hip.CtcSegmentArgs()
    fake = 1 << 12
    a.logits, a.ldv, a.B, a.T, a.V = fake, 40, 2, 100, 37
    a.hlens, a.targets, a.Lmax, a.tlens = fake, fake, 9, fake
    a.free_start, a.free_end = 1, 1
    a.frames, a.score, a.workspace = fake, fake, fake
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("change,word", [(dict(frames=None), b"null"), (dict(score=None), b"null"), (dict(workspace=None), b"null"),
                                         (dict(logits=None), b"null"), (dict(targets=None), b"null targets"),
                                         (dict(Lmax=8192), b"8191-label limit"), (dict(T=0), b"bad shape"),
                                         (dict(T=(1 << 20) + 1), b"bad shape"), (dict(ldv=36), b"bad shape"), (dict(B=0), b"bad shape"),
                                         (dict(V=1), b"bad shape"), (dict(Lmax=-1), b"bad shape")])
def test_segment_refuses_before_any_launch(change, word):
    from openeat_amd import hip
    lib = hip.lib()
    a = seg_args(**change)
    rc = lib.oe_ctc_segment(C.byref(a), None)
    assert rc != 0 and word in lib.oe_last_error(), lib.oe_last_error()


def test_segment_refuses_null_args():
    from openeat_amd import hip
    lib = hip.lib()
    assert lib.oe_ctc_segment(None, None) != 0 and b"null args" in lib.oe_last_error()


@pytest.mark.parametrize("B,T,V,Lmax", [(1, 45000, 4233, 7000), (8, 45000, 4233, 7000), (1, 2 ** 20, 16, 8191), (1, 1, 2, 8191), (3, 1, 2, 0),
                                         (2, 700, 40, 2047), (2, 700, 40, 2048), (2, 700, 40, 4095), (2, 700, 40, 4096), (1, 5, 2, 64)])
def test_workspace_bound(B, T, V, Lmax):
    """No float per cell: at most 4 bits per cell, a T x V float matrix and per-frame bookkeeping."""
    from openeat_amd import hip
    n = hip.lib().oe_ctc_segment_workspace_bytes(B, T, V, Lmax)
    Sp = (2 * Lmax + 1 + 127) // 128 * 128
    assert 0 < n <= B * (T * (Sp // 2 + 4 * V + 64) + 65536)
    assert n >= B * T * (2 * Lmax + 1) // 4                               # 2 bits for every cell are there
    print(f"B={B} T={T} V={V} Lmax={Lmax}: {n} bytes = {8 * n / (B * T * (2 * Lmax + 1)):.2f} bits per cell")


def test_workspace_bytes_is_zero_outside_the_limits():
    from openeat_amd import hip
    f = hip.lib().oe_ctc_segment_workspace_bytes
    assert f(1, 100, 37, 8192) == 0 and f(0, 100, 37, 9) == 0 and f(1, 0, 37, 9) == 0 and f(1, (1 << 20) + 1, 37, 9) == 0
