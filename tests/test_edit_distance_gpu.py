"""GPU: batched edit distance (oe_edit_distance) through the C ABI against the plain-Python yardstick (edit_distance_ref.py, which
test_edit_distance_ref.py pins to what the reference's error-rate tool answered), and through ops.edit_distance,
ASRModel.error_counts and Executor.cv.  Every output is an integer and every comparison is exact equality.

Raw calls use leading dimensions above the maxima, fill what lies behind a row's length with tokens of the OTHER sequence (an
over-read would find matches) and prefill the outputs with a sentinel (an unwritten cell shows).  At most five pairs above
300 tokens in the whole file: the yardstick is a Python loop.

The file is not named test_gpu_*: conftest.py orders those files by a fixed list that test_host_logic.py holds complete.
"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edit_distance_ref as R  # noqa: E402
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
SENTINEL = -77


def _poison(other, length):
    """`length` tokens that occur in `other` (cyclic), so that reading behind a row's end finds matches."""
    return [other[k % len(other)] for k in range(length)] if other else [0] * length


def run_raw(refs, hyps, group=1, align=True, Nmax=None, Mmax=None, pad=3):
    """refs: U token lists, hyps: U * group token lists or None (the slot does not exist) -> (counts (P, 4), ref_to_hyp (P, Nmax)
    or None, workspace bytes) as numpy."""
    P, U = len(hyps), len(refs)
    assert U * group == P
    Nmax = max(len(r) for r in refs) if Nmax is None else Nmax
    Mmax = max(len(h) for h in hyps if h is not None) if Mmax is None else Mmax
    ref_ld, hyp_ld = Nmax + pad, Mmax + pad
    ref_m = np.zeros((U, ref_ld), dtype=np.int32)
    hyp_m = np.zeros((P, hyp_ld), dtype=np.int32)
    for u, r in enumerate(refs):
        other = next((h for h in hyps[u * group:(u + 1) * group] if h), [])
        ref_m[u] = list(r) + _poison(other, ref_ld - len(r))
    for p, h in enumerate(hyps):
        r = refs[p // group]
        hyp_m[p] = _poison(r, hyp_ld) if h is None else list(h) + _poison(r, hyp_ld - len(h))
    rl = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=DEV)
    hl = torch.tensor([-1 if h is None else len(h) for h in hyps], dtype=torch.int32, device=DEV)
    ref_d, hyp_d = torch.from_numpy(ref_m).to(DEV), torch.from_numpy(hyp_m).to(DEV)
    counts = torch.full((P, 4), SENTINEL, dtype=torch.int32, device=DEV)
    r2h = torch.full((P, Nmax), SENTINEL, dtype=torch.int32, device=DEV) if align else None
    L = hip.lib()
    nbytes = L.oe_edit_distance_workspace_bytes(P, Nmax, Mmax) if align else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    hip.check(L.oe_edit_distance(hip.ptr(ref_d), ref_ld, hip.ptr(rl), group, hip.ptr(hyp_d), hyp_ld, hip.ptr(hl), P, Nmax, Mmax,
                                 hip.ptr(counts), hip.ptr(r2h), hip.ptr(ws), hip.stream()), "oe_edit_distance")
    torch.cuda.synchronize()
    return counts.cpu().numpy(), None if r2h is None else r2h.cpu().numpy(), nbytes


def yardstick(refs, hyps, group=1):
    return [None if h is None else R.edit_distance(refs[p // group], h) for p, h in enumerate(hyps)]


def check(want, refs, counts, r2h, group=1):
    for p, w in enumerate(want):
        n = len(refs[p // group])
        if w is None:
            assert counts[p].tolist() == [-1] * 4, p
            if r2h is not None:
                assert (r2h[p] == -1).all(), p
            continue
        assert tuple(counts[p].tolist()) == w[0], (p, n, counts[p].tolist(), w[0])
        if r2h is not None:
            assert r2h[p, :n].tolist() == w[1], (p, n)
            assert (r2h[p, n:] == -1).all(), (p, n)


def both_ways(refs, hyps, group=1, **kw):
    """Aligned and counts-only calls against the yardstick; the two must return the same counts."""
    want = yardstick(refs, hyps, group)
    counts, r2h, nbytes = run_raw(refs, hyps, group, True, **kw)
    check(want, refs, counts, r2h, group)
    only, _, _ = run_raw(refs, hyps, group, False, **kw)
    assert np.array_equal(only, counts)
    return want, counts, r2h, nbytes


def draw(rng, n, vocab=3):
    return [rng.randrange(vocab) for _ in range(n)]


def test_lane_and_cells_per_lane_edges_in_one_launch():
    """Every (n, m) of the lane-count and cells-per-lane edges, vocabulary 3 (ties are dense), back-pointers in LDS."""
    rng = random.Random(1)
    sizes = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
    refs = [draw(rng, n) for n in sizes for _ in sizes]
    hyps = [draw(rng, m) for _ in sizes for m in sizes]
    want, counts, r2h, nbytes = both_ways(refs, hyps, Nmax=257, Mmax=257)
    assert nbytes == 0
    assert sum(w[0][1] + w[0][2] + w[0][3] > 0 for w in want) >= 140


def test_longest_pairs_keep_back_pointers_in_the_workspace():
    """Nmax = Mmax = 1023: sixteen cells per lane and the workspace route, for the longest pairs and for short ones beside them."""
    rng = random.Random(2)
    same = draw(rng, 1023)
    refs = [draw(rng, 1023), draw(rng, 1023), [], same, draw(rng, 1023)]
    hyps = [draw(rng, 1023), draw(rng, 1), draw(rng, 1023), list(same), [3 + t for t in draw(rng, 700)]]      # the last: no token in common
    for n, m in ((1, 1), (5, 0), (0, 0), (17, 40), (64, 65), (130, 7), (3, 200), (255, 256), (1, 300), (300, 2)):
        refs.append(draw(rng, n))
        hyps.append(draw(rng, m))
    want, counts, r2h, nbytes = both_ways(refs, hyps, Nmax=1023, Mmax=1023)
    assert nbytes == len(hyps) * 1023 * 64 * 4
    assert counts[3].tolist() == [1023, 0, 0, 0] and r2h[3].tolist() == list(range(1023))
    assert counts[2].tolist() == [0, 0, 0, 1023]
    assert counts[4, 0] == 0 and counts[4].tolist()[1:] == [700, 323, 0]


@pytest.mark.parametrize("Nmax,Mmax", [(9, 33), (64, 64), (100, 150), (128, 17), (200, 64), (256, 1), (300, 120), (40, 0), (0, 40)])
def test_every_cells_per_lane_class(Nmax, Mmax):
    rng = random.Random(Nmax * 1000 + Mmax)
    ns = [Nmax, Nmax, max(Nmax - 1, 0), Nmax // 2, 0, 1] + [rng.randrange(Nmax + 1) for _ in range(6)]
    ms = [Mmax, max(Mmax - 1, 0), Mmax, 1, Mmax // 2, 0] + [rng.randrange(Mmax + 1) for _ in range(6)]
    refs = [draw(rng, min(n, Nmax)) for n in ns]
    hyps = [draw(rng, min(m, Mmax)) for m in ms]
    both_ways(refs, hyps, Nmax=Nmax, Mmax=Mmax)


@pytest.mark.parametrize("Mmax,in_lds", [(192, True), (193, False)])
def test_either_side_of_the_lds_limit(Mmax, in_lds):
    """Nmax = 1023: 12 words a row are 49 104 bytes of back-pointers, the largest LDS launch; 13 words go to the workspace.  The
    route depends on the maxima only, so the pairs themselves stay short."""
    rng = random.Random(Mmax)
    ns = (300, 299, 1, 0, 64, 130, 257, 17)
    ms = (Mmax, Mmax - 1, Mmax, 5, 0, 177, 16, Mmax)
    refs, hyps = [draw(rng, n) for n in ns], [draw(rng, m) for m in ms]
    _, _, _, nbytes = both_ways(refs, hyps, Nmax=1023, Mmax=Mmax)
    assert (nbytes == 0) == in_lds and nbytes in (0, len(hyps) * 1023 * 13 * 4)


def test_hand_worked_tie_cases_on_the_device():
    """The pairs of test_edit_distance_ref.py::test_tie_order_decides_the_counts, where the tie order decides the counts."""
    a, b = 7, 9
    refs = [[a, b], [a], [a, a], [a], [a, b, a], [], [a, b], []]
    hyps = [[b, a], [b, b], [a], [a, a], [b], [], [], [a, b, a]]
    want = [((1, 0, 1, 1), [1, -1]), ((0, 1, 0, 1), [0]), ((1, 0, 1, 0), [0, -1]), ((1, 0, 0, 1), [0]), ((1, 0, 2, 0), [-1, 0, -1]),
            ((0, 0, 0, 0), []), ((0, 0, 2, 0), [-1, -1]), ((0, 0, 0, 3), [])]
    counts, r2h, _ = run_raw(refs, hyps)
    check(want, refs, counts, r2h)
    only, _, _ = run_raw(refs, hyps, align=False)
    assert np.array_equal(only, counts)


def test_device_lengths_above_the_maxima_are_clamped():
    """The lengths live on the device: the kernel cuts one above its maximum (the rows here do hold that many tokens)."""
    rng = random.Random(3)
    refs, hyps = [draw(rng, 20), draw(rng, 12)], [draw(rng, 15), draw(rng, 20)]
    counts, r2h, _ = run_raw(refs, hyps, Nmax=16, Mmax=10, pad=12)
    want0 = R.edit_distance(refs[0][:16], hyps[0][:10])
    assert tuple(counts[0].tolist()) == want0[0] and r2h[0].tolist() == want0[1]
    want1 = R.edit_distance(refs[1], hyps[1][:10])
    assert tuple(counts[1].tolist()) == want1[0] and r2h[1, :12].tolist() == want1[1] and (r2h[1, 12:] == -1).all()


def test_nbest_lists_against_their_utterance_and_the_oracle():
    from openeat_amd.utils.error_rate import ErrorRate, nbest_oracle
    rng = random.Random(4)
    U, beam = 8, 4
    refs = [draw(rng, n, 5) for n in (12, 30, 7, 0, 25, 18, 40, 9)]
    hyps = []
    for u, r in enumerate(refs):
        for k in range(beam):
            h = [t for t in r if rng.random() > 0.15 * k]                   # later slots lose more tokens
            if rng.random() < 0.5:
                h.insert(rng.randrange(len(h) + 1), rng.randrange(5))
            hyps.append(h)
    absent = {0 * beam + 3, 1 * beam + 0, 2 * beam + 1, 2 * beam + 2, 4 * beam + 0, 4 * beam + 1, 4 * beam + 2,      # utterance 4: only the last
              6 * beam + 0, 6 * beam + 1, 6 * beam + 2, 6 * beam + 3}                                                # utterance 6: none at all
    hyps[5 * beam + 2] = list(hyps[5 * beam + 0])                           # utterance 5: slots 0 and 2 tie ...
    hyps[5 * beam + 1] = hyps[5 * beam + 0] + [1, 2, 3]                     # ... and 1 is worse
    hyps[5 * beam + 3] = [4] + hyps[5 * beam + 0] + [0, 0]
    hyps[7 * beam + 0] = [9, 9, 9]                                           # utterance 7: the best is not the first
    hyps[7 * beam + 1] = list(refs[7][:-1])
    hyps[7 * beam + 2] = list(refs[7])
    hyps = [None if p in absent else h for p, h in enumerate(hyps)]
    want, counts, r2h, _ = both_ways(refs, hyps, group=beam, Nmax=40, Mmax=45)
    best, index = nbest_oracle(torch.from_numpy(counts).to(DEV), beam)
    best, index = best.cpu().tolist(), index.cpu().tolist()
    for u in range(U):
        errs = [None if w is None else sum(w[0][1:]) for w in want[u * beam:(u + 1) * beam]]
        have = [e for e in errs if e is not None]
        if not have:
            assert index[u] == 0 and best[u] == [-1] * 4
            continue
        assert index[u] == errs.index(min(have)), (u, errs, index[u])        # list.index: the lowest index among equals
        assert tuple(best[u]) == want[u * beam + index[u]][0]
    assert index[4] == 3 and index[5] == 0 and index[7] == 2
    er = ErrorRate().update(torch.from_numpy(counts).to(DEV))
    tot = [sum(w[0][k] for w in want if w is not None) for k in range(4)]
    assert er.result() == {"all": tot[0] + tot[1] + tot[2], "cor": tot[0], "sub": tot[1], "del": tot[2], "ins": tot[3],
                           "rate": (tot[1] + tot[2] + tot[3]) / (tot[0] + tot[1] + tot[2])}


@pytest.mark.parametrize("n", [40, 100, 150, 300])
def test_planted_edits_come_back_exactly(n):
    """Unique tokens and edits kept apart by untouched tokens: the optimal alignment is unique and known without any DP."""
    rng = random.Random(n)
    ref = rng.sample(range(1000, 5000), n)
    fresh = iter(range(10000, 20000))
    slots = list(range(1, n - 1, 3))                                        # at least two untouched tokens between edits
    rng.shuffle(slots)
    k = len(slots) // 4
    dele, sub, ins_before = set(slots[:k]), set(slots[k:2 * k]), set(slots[2 * k:3 * k])
    hyp, r2h = [], []
    for i, t in enumerate(ref):
        if i in ins_before:
            hyp.append(next(fresh))
        if i in dele:
            r2h.append(-1)
            continue
        r2h.append(len(hyp))
        hyp.append(next(fresh) if i in sub else t)
    counts, got, _ = run_raw([ref], [hyp])
    assert counts[0].tolist() == [n - 2 * k, k, k, k]
    assert got[0].tolist() == r2h
    assert R.edit_distance(ref, hyp) == ((n - 2 * k, k, k, k), r2h)
    only, _, _ = run_raw([ref], [hyp], align=False)
    assert np.array_equal(only, counts)


def _pad(rows, width, fill=-1, dtype=torch.int64):
    out = torch.full((len(rows), width), fill, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, : len(r)] = torch.tensor(r, dtype=dtype)
    return out


def test_ops_edit_distance_surface():
    from openeat_amd import ops
    rng = random.Random(5)
    refs = [draw(rng, n) for n in (11, 0, 30, 30)]
    hyps = [draw(rng, m) for m in (9, 4, 0, 33)]
    want = yardstick(refs, hyps)
    rl, hl = torch.tensor([len(r) for r in refs]), torch.tensor([len(h) for h in hyps])
    for dtype in (torch.int64, torch.int32, torch.int16):
        counts, r2h = ops.edit_distance(_pad(refs, 30, 1, dtype).to(DEV), rl.to(dtype).to(DEV), _pad(hyps, 35, 2, dtype).to(DEV),
                                        hl.to(dtype).to(DEV), align=True)
        assert counts.dtype == r2h.dtype == torch.int32 and counts.shape == (4, 4) and r2h.shape == (4, 30)
        check(want, refs, counts.cpu().numpy(), r2h.cpu().numpy())
        only = ops.edit_distance(_pad(refs, 30, 1, dtype).to(DEV), rl.to(DEV), _pad(hyps, 35, 2, dtype).to(DEV), hl.to(DEV))
        assert torch.equal(only, counts)
    # no columns at all on either side
    z = torch.zeros(4, dtype=torch.int64, device=DEV)
    counts, r2h = ops.edit_distance(torch.zeros(4, 0, dtype=torch.int64, device=DEV), z, _pad(hyps, 35, 2).to(DEV), hl.to(DEV), align=True)
    assert r2h.shape == (4, 0) and counts.cpu().tolist() == [[0, 0, 0, len(h)] for h in hyps]
    counts, r2h = ops.edit_distance(_pad(refs, 30, 1).to(DEV), rl.to(DEV), torch.zeros(4, 0, dtype=torch.int64, device=DEV), z, align=True)
    assert counts.cpu().tolist() == [[0, 0, len(r), 0] for r in refs] and bool((r2h == -1).all())
    counts = ops.edit_distance(torch.zeros(4, 0, dtype=torch.int64, device=DEV), z, torch.zeros(4, 0, dtype=torch.int64, device=DEV), z)
    assert counts.cpu().tolist() == [[0, 0, 0, 0]] * 4
    # no pairs: empty tensors, nothing launched
    e = torch.zeros(0, 7, dtype=torch.int64, device=DEV)
    counts, r2h = ops.edit_distance(e, z[:0], e, z[:0], align=True)
    assert counts.shape == (0, 4) and r2h.shape == (0, 7)
    with pytest.raises(TypeError, match="CUDA tensors"):
        ops.edit_distance(_pad(refs, 30), rl, _pad(hyps, 35), hl)
    with pytest.raises(TypeError, match="integer tensors"):
        ops.edit_distance(_pad(refs, 30).float().to(DEV), rl.to(DEV), _pad(hyps, 35).to(DEV), hl.to(DEV))
    with pytest.raises(ValueError, match="group"):
        ops.edit_distance(_pad(refs, 30).to(DEV), rl.to(DEV), _pad(hyps, 35).to(DEV), hl.to(DEV), group=2)
    with pytest.raises(RuntimeError, match="1023-token limit"):
        ops.edit_distance(torch.zeros(1, 1024, dtype=torch.int64, device=DEV), z[:1], _pad(hyps[:1], 35).to(DEV), hl[:1].to(DEV))


def test_edit_distance_captured_in_a_graph_replays_bit_for_bit():
    from openeat_amd import ops
    g0 = torch.Generator().manual_seed(6)
    U, beam, Nmax, Mmax = 6, 3, 70, 90

    def batch():
        hl = torch.randint(0, Mmax + 1, (U * beam,), generator=g0)
        hl[torch.randperm(U * beam, generator=g0)[:4]] = -1                  # four slots do not exist, elsewhere in every batch
        return (torch.randint(0, 4, (U, Nmax), generator=g0).to(DEV), torch.randint(0, Nmax + 1, (U,), generator=g0).to(DEV),
                torch.randint(0, 4, (U * beam, Mmax), generator=g0).to(DEV), hl.to(DEV))

    static = batch()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.edit_distance(*static, group=beam, align=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = ops.edit_distance(*static, group=beam, align=True)
            only = ops.edit_distance(*static, group=beam)
    torch.cuda.current_stream().wait_stream(s)
    first = None
    for _ in range(2):
        fresh = batch()
        for a, b in zip(static, fresh):
            a.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.edit_distance(*[t.clone() for t in fresh], group=beam, align=True)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1]) and torch.equal(only, eager[0])
        assert first is None or not torch.equal(first, eager[0])
        first = eager[0].clone()
    refs = [fresh[0][u, : int(fresh[1][u])].tolist() for u in range(U)]
    hyps = [None if int(fresh[3][p]) < 0 else fresh[2][p, : int(fresh[3][p])].tolist() for p in range(U * beam)]
    assert any(h is None for h in hyps)
    check(yardstick(refs, hyps, beam), refs, outs[0].cpu().numpy(), outs[1].cpu().numpy(), beam)


# ------------------------------------------------------------------ model level --
def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), {k: v.to(DEV) for k, v in g["in"].items()}


def _targets_near(lists, seed, vocab):
    """One target per decoded list: the list with a token dropped, one replaced and one added (so cor, sub, del and ins all
    occur), except utterance 1, whose target is empty."""
    rng = random.Random(seed)
    out = []
    for b, h in enumerate(lists):
        t = list(h)
        if t:
            del t[rng.randrange(len(t))]
        if t:
            t[rng.randrange(len(t))] = 1 + rng.randrange(vocab - 2)
        t.insert(rng.randrange(len(t) + 1), 1 + rng.randrange(vocab - 2))
        out.append([] if b == 1 else t)
    return out


def _model_batches():
    """The golden batch, and the same features with utterance 0 cut to a shorter features_length."""
    model, i = tiny_conformer()
    feats, flen = i["feats"], i["flen"]
    short = flen.clone()
    short[0] = int(flen[0]) * 2 // 3
    return model, feats, [flen, short]


def test_model_error_counts_greedy():
    model, feats, flens = _model_batches()
    for k, flen in enumerate(flens):
        with torch.no_grad():
            lists = model.ctc_greedy_search(feats, flen)
        tgt = _targets_near(lists, 20 + k, model.vocab_size)
        width = max(len(t) for t in tgt) + 2
        out = model.error_counts(feats, flen, _pad(tgt, width).to(DEV), torch.tensor([len(t) for t in tgt]).to(DEV))
        assert set(out) == {"counts"} and out["counts"].is_cuda and out["counts"].dtype == torch.int32
        want = [R.edit_distance(t, h)[0] for t, h in zip(tgt, lists)]
        assert [tuple(r) for r in out["counts"].cpu().tolist()] == want
        assert want[1] == (0, 0, 0, len(lists[1]))
    with pytest.raises(ValueError):
        model.error_counts(feats, flens[0], _pad(tgt, width).to(DEV), torch.tensor([len(t) for t in tgt]).to(DEV), nbest_oracle=True)


def test_model_error_counts_attention_rescoring_and_oracle():
    model, feats, flens = _model_batches()
    beam = 4
    for k, flen in enumerate(flens):
        lists = model.attention_rescoring_batch(feats, flen, beam)
        tgt = _targets_near(lists, 30 + k, model.vocab_size)
        tg, tl = _pad(tgt, max(len(t) for t in tgt) + 1).to(DEV), torch.tensor([len(t) for t in tgt]).to(DEV)
        out = model.error_counts(feats, flen, tg, tl, mode="attention_rescoring", beam_size=beam, nbest_oracle=True)
        assert set(out) == {"counts", "oracle_counts", "oracle_index"} and all(v.is_cuda for v in out.values())
        want = [R.edit_distance(t, h)[0] for t, h in zip(tgt, lists)]
        counts = [tuple(r) for r in out["counts"].cpu().tolist()]
        assert counts == want
        plain = model.error_counts(feats, flen, tg, tl, mode="attention_rescoring", beam_size=beam)
        assert set(plain) == {"counts"} and torch.equal(plain["counts"], out["counts"])
        with torch.no_grad():
            _, _, pre, plen, _, _, _ = model._rescore_stage1(feats, flen, hip.PrefixSearch(beam))
        pre, plen = pre.cpu(), plen.cpu().tolist()
        oracle, index = out["oracle_counts"].cpu().tolist(), out["oracle_index"].cpu().tolist()
        for b, t in enumerate(tgt):
            slots = [None if plen[b * beam + s] < 0 else R.edit_distance(t, pre[b * beam + s, : plen[b * beam + s]].tolist())[0]
                     for s in range(beam)]
            errs = [None if c is None else sum(c[1:]) for c in slots]
            best = min(e for e in errs if e is not None)
            assert index[b] == errs.index(best) and tuple(oracle[b]) == slots[index[b]]
            assert sum(oracle[b][1:]) == best <= sum(counts[b][1:])


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def test_executor_cv_reports_the_token_error_rate():
    from openeat_amd.utils.error_rate import overall_line
    from openeat_amd.utils.executor import Executor
    model, feats, flens = _model_batches()
    loader = []
    tot = [0, 0, 0, 0]
    for k, flen in enumerate(flens):
        with torch.no_grad():
            lists = model.ctc_greedy_search(feats, flen)
        tgt = [t if t else [3] for t in _targets_near(lists, 40 + k, model.vocab_size)]       # the training loss wants a label
        for t, h in zip(tgt, lists):
            for j, c in enumerate(R.edit_distance(t, h)[0]):
                tot[j] += c
        loader.append(([f"utt{k}_{b}" for b in range(len(tgt))],
                       {"features": feats.cpu(), "features_length": flen.cpu(), "targets": _pad(tgt, max(len(t) for t in tgt)),
                        "targets_length": torch.tensor([len(t) for t in tgt])}))
    runs = {}
    for name, args in (("absent", {"log_interval": 1}), ("false", {"log_interval": 1, "cv_error_rate": False}),
                       ("on", {"log_interval": 1, "cv_error_rate": True})):
        ex, log = Executor(), _Log()
        runs[name] = (ex, log.lines, ex.cv(log, model, loader, torch.device(DEV), args))
    ex, lines, pair = runs["on"]
    want = {"all": tot[0] + tot[1] + tot[2], "cor": tot[0], "sub": tot[1], "del": tot[2], "ins": tot[3],
            "rate": (tot[1] + tot[2] + tot[3]) / (tot[0] + tot[1] + tot[2])}
    assert ex.last_cv_error_rate == want
    ter = [l for l in lines if l.startswith("CV TER ")]
    assert ter == ["CV TER " + overall_line(want)] and lines[-1] == ter[0]
    for name in ("absent", "false"):
        ex_off, lines_off, pair_off = runs[name]
        assert not hasattr(ex_off, "last_cv_error_rate")
        assert lines_off == lines[:-1] and len(lines_off) == 2 and all(l.startswith("CV Batch[") for l in lines_off)
        assert pair_off == pair and isinstance(pair_off, tuple) and len(pair_off) == 2
