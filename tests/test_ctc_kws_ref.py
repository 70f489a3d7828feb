"""CPU: the restatement of keyword search over CTC posteriors (ctc_kws_ref.py) against a fixed-span DP over every start frame,
its tie rules on hand-worked cases, its float32 run against its float64 run on the fixtures the GPU tests use (the 1/8-grid
ones, where every float32 sum is exact, and the continuous ones, where equal spans are a condition on the seeds), the keyword
list of openeat_amd/utils/keyword.py, and what oe_ctc_kws refuses through the loaded library (no device is touched: every call
here returns before any launch)."""
import ctypes as C

import numpy as np
import pytest

import ctc_kws_ref as R
from openeat_amd.utils.keyword import KeywordList, hit_records

LOG_HALF = float(np.float32(np.log(0.5)))


def test_carried_start_against_a_fixed_span_dp_over_every_start():
    rng = np.random.default_rng(1)
    cases = 0
    for L in (1, 2, 3):
        for rep in range(12):
            T, V = int(rng.integers(L, 13)), int(rng.integers(3, 6))
            y = [int(c) for c in rng.integers(1, V, size=L)]
            if rep % 3 == 0 and L > 1:
                y[1] = y[0]
            lp = R.log_softmax(rng.standard_normal((T, V)) * 2)
            cands = {t: (st, sc) for t, st, sc in R.candidates(lp, y)}
            for t in range(T):
                spans = [R.span_optimum(lp, y, a, t) for a in range(t + 1)]
                want = max(spans)
                if want == -np.inf:
                    assert t not in cands
                    continue
                st, sc = cands[t]
                assert sc == pytest.approx(want, rel=1e-12, abs=1e-12)
                assert spans[st] == pytest.approx(want, rel=1e-12, abs=1e-12), (y, t, st)
                cases += 1
    assert cases > 150


def test_stay_and_fresh_tie_at_zero_keeps_the_earlier_start():
    """One label with lp 0 on frames 0 and 1: at t = 1 and at t = 2 stay (0) and fresh (0) tie, stay was tried first, so the
    start stays 0 and the candidates span two and three frames.  At t = 3 stay is -1 < 0 and fresh wins."""
    lp = np.array([[-5.0, 0.0], [-5.0, 0.0], [-5.0, -1.0], [-5.0, 0.0]])
    assert R.candidates(lp, [1]) == [(0, 0, 0.0), (1, 0, 0.0), (2, 0, -1.0), (3, 3, 0.0)]
    hits, best = R.search_one(lp, [1], -0.5)
    # (0,0) pending; (0,1) overlaps, mean 0 = 0: not better; (0,2) passes (-1 >= -1.5), overlaps, worse; (3,3) does not overlap
    assert hits == [(0, 0, 0.0), (3, 3, 0.0)] and best == (0, 0, 0.0)


def test_two_candidates_that_tie_in_mean_score_keep_the_earlier():
    """Keyword (1, 2): candidates (0..1, -1/2) and (0..3, -1): both mean -1/4 per frame, compared as -0.5 * 4 > -1 * 2: false."""
    lp = np.full((4, 3), -8.0)
    lp[0, 1] = -0.25
    lp[1, 2] = -0.25                 # candidate at t = 1: span [0, 1], sc -0.5
    lp[2, 2] = -0.25
    lp[3, 2] = -0.25                 # candidate at t = 3: span [0, 3], sc -1.0
    cands = R.candidates(lp, [1, 2])
    assert cands == [(1, 0, -0.5), (2, 0, -0.75), (3, 0, -1.0)]
    assert not R.better(-1.0, 4, -0.5, 2) and not R.better(-0.5, 2, -1.0, 4) and not R.better(-0.75, 3, -0.5, 2)
    hits, best = R.search_one(lp, [1, 2], -0.25)
    assert hits == [(0, 1, -0.5)] and best == (0, 1, -0.5)
    hits, _ = R.search_one(lp, [1, 2], -0.2)
    assert hits == []


def grid_cases(n=60):
    rng = np.random.default_rng(7)
    for i in range(n):
        V, T, L = int(rng.integers(3, 9)), int(rng.integers(20, 201)), int(rng.integers(1, 6))
        y = [int(c) for c in rng.integers(1, V, size=L)]
        yield R.grid_case(rng, T, V), y


def test_grid_fixtures_run_identically_in_float32():
    n_hits = n_cands = 0
    for lp, y in grid_cases():
        c64, c32 = R.candidates(lp, y), R.candidates(lp, y, np.float32)
        assert [(t, s, float(v)) for t, s, v in c32] == c64
        h64, b64 = R.scan(c64, -0.5)
        h32, b32 = R.scan(c32, -0.5)
        assert h64 == [(s, e, float(v)) for s, e, v in h32] and b64 == (b32[0], b32[1], float(b32[2]))
        n_hits, n_cands = n_hits + len(h64), n_cands + len(c64)
    print(f"{n_hits} hits, {n_cands} candidates")
    assert n_hits > 300 and n_cands > 2000


@pytest.mark.parametrize("seed", R.RAW_SEEDS)
def test_continuous_fixtures_give_the_same_spans_in_float32(seed):
    """A condition on the inputs: the seeds the GPU test uses are chosen so that it holds."""
    logits, kws, planted = R.raw_fixture(seed)
    lp64 = R.log_softmax(logits)
    lp32 = lp64.astype(np.float32)
    total = 0
    for k, y in enumerate(kws):
        h64, b64 = R.search_one(lp64, y, LOG_HALF)
        h32, b32 = R.search_one(lp32, y, LOG_HALF, np.float32)
        assert [(s, e) for s, e, _ in h64] == [(s, e) for s, e, _ in h32], (seed, k)
        assert b64[:2] == b32[:2]
        total += len(h64)
        for kk, s, e in planted:
            if kk == k:
                assert (s, e) in [(a, b) for a, b, _ in h64], (seed, k, s, e, h64)
    assert len(planted) >= 3 and 3 <= total < logits.shape[0]


def test_keyword_list_tables_and_records():
    kl = KeywordList([[5, 3, 5], [9], [3, 9, 9, 2]], thresholds=[0.5, 1.0, 1e-6])
    assert kl.cols.tolist() == [2, 3, 5, 9] and kl.klens.tolist() == [3, 1, 4]
    assert kl.kw_col.tolist() == [[2, 1, 2, 0], [3, 0, 0, 0], [1, 3, 3, 0]]
    assert kl.log_thr.dtype == np.float32 and kl.log_thr[1] == 0.0 and kl.log_thr[0] == np.float32(np.log(0.5))
    assert kl.group_bounds(3) == [0, 2, 3] and kl.group_bounds(1) == [0, 1, 2, 3] and kl.group_bounds(4) == [0, 3]
    sub = kl.subset(1, 3)
    assert sub.phrases == kl.phrases[1:] and sub.log_thr.tolist() == kl.log_thr[1:].tolist() and sub.cols.tolist() == [2, 3, 9]
    t2i = {"a": 1, "b": 2, "c": 3, "_": 0}
    txt = KeywordList.from_text(["ab c", "", "abc", "a_", "zz", "ca"], t2i, threshold=0.25)
    assert txt.phrases == [(1, 2, 3), (3, 1)] and txt.skipped == 2 and txt.confidence == [0.25, 0.25]
    for bad in (dict(phrases=[]), dict(phrases=[[]]), dict(phrases=[[1] * 33]), dict(phrases=[[1]], threshold=0.0),
                dict(phrases=[[1]], thresholds=[0.5, 0.5])):
        with pytest.raises(ValueError):
            KeywordList(**bad)
    recs, trunc = hit_records(kl, [[1, 0, 3]], [[[7, -1], [-1, -1], [2, 11]]], [[[9, -1], [-1, -1], [5, 12]]],
                              [[[-1.5, 0.0], [0.0, 0.0], [-2.0, -0.5]]], times=lambda s, e: (s * 0.04, (e + 1) * 0.04))
    assert trunc == [[False, False, True]]
    assert [(r["keyword"], r["start_frame"], r["end_frame"]) for r in recs[0]] == [(2, 2, 5), (0, 7, 9), (2, 11, 12)]
    assert recs[0][1] == {"keyword": 0, "tokens": [5, 3, 5], "start_frame": 7, "end_frame": 9, "score": -1.5,
                          "confidence": float(np.exp(-0.5)), "start_s": 7 * 0.04, "end_s": 10 * 0.04}


def kws_args(hip, **over):
    """Arguments that pass every check but point nowhere a launch could use: only calls that are refused are made with them."""
    q = hip.KeywordSet(0x1000, 3, 0x1000, 0x1000, 0x1000, 2, 4)
    a = hip.CtcKwsArgs()
    a.logits, a.ldv, a.B, a.T, a.V, a.hlens = 0x1000, 8, 1, 10, 8, 0x1000
    a.normalized, a.max_hits = 0, 2
    a.n_hits = a.hit_start = a.hit_end = a.hit_score = a.workspace = 0x1000
    for name, val in over.items():
        if hasattr(q, name) and name not in ("T", "B", "V"):
            setattr(q, name, val)
        else:
            setattr(a, name, val)
    a.kws = C.pointer(q)
    return a


@pytest.mark.parametrize("over,text", [(dict(K=0), b"K=0"), (dict(K=65536), b"K=65536"), (dict(Lmax=33), b"Lmax=33"), (dict(Lmax=0), b"Lmax=0"),
                                       (dict(U=8), b"U=8"), (dict(U=0), b"U=0"), (dict(hlens=None), b"hlens"), (dict(logits=None), b"logits"),
                                       (dict(thr=None), b"thr"), (dict(hit_score=None), b"hit_score"), (dict(workspace=None), b"workspace"),
                                       (dict(T=(1 << 20) + 1), b"T=1048577"), (dict(max_hits=0), b"max_hits=0"), (dict(ldv=7), b"ldv=7")])
def test_bad_arguments_are_refused_before_any_launch(over, text):
    from openeat_amd import hip
    lib = hip.lib()
    rc = lib.oe_ctc_kws(C.byref(kws_args(hip, **over)), None)
    assert rc != 0 and text in lib.oe_last_error(), lib.oe_last_error()


def test_workspace_bytes_and_abi_version():
    from openeat_amd import hip
    lib = hip.lib()
    assert lib.oe_abi_version() >= 6
    assert lib.oe_ctc_kws_workspace_bytes(3, 1000, 50) == 3 * 1000 * 51 * 4
    assert lib.oe_ctc_kws_workspace_bytes(1, 90000, 4232) == 90000 * 4233 * 4                # beyond 2^31
    for B, T, U in ((0, 10, 5), (1, 0, 5), (1, (1 << 20) + 1, 5), (1, 10, 0)):
        assert lib.oe_ctc_kws_workspace_bytes(B, T, U) == 0
