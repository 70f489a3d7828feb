"""GPU: keyword search over CTC posteriors (oe_ctc_kws) through the C ABI against the restatement (ctc_kws_ref.py), and through
ops.ctc_keyword_search / ASRModel.keyword_search.

Exact mode (normalized=1): log-probabilities on the 1/8 grid, where every float32 sum is exact (test_ctc_kws_ref.py shows the
restatement's float32 run identical to its float64 run there), so every output must EQUAL the float64 restatement bit for bit,
unused slots included.  Raw mode (normalized=0): continuous logits; the device's hits are held to the aligner's tolerance
(rtol 1e-4 / atol 1e-3, as test_ctc_align_gpu.py) against float64 optima, never to equal spans except for planted occurrences.

The kernel runs 4 keywords per workgroup (K = 5 and 9 are one more than a multiple) and loads 16 frames ahead of the recursion
(T = 15, 16, 17 are one below, at and one above).

Not named test_gpu_*: conftest.py orders those files by a fixed list."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_kws_ref as R  # noqa: E402
from openeat_amd import hip  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-3
LOG_HALF = float(np.float32(np.log(0.5)))
SENT_I, SENT_F = -7, 5.0
NAMES = ("n_hits", "hit_start", "hit_end", "hit_score", "best_start", "best_end", "best_score")


def tables(keywords, Lmax=None):
    """cols, kw_col, klens of a list of label lists as the kernel reads them (labels as given: none is checked here)."""
    cols = sorted({int(t) for y in keywords for t in y})
    index = {t: i for i, t in enumerate(cols)}
    Lmax = Lmax or max(max(len(y) for y in keywords), 1)
    kw_col = np.zeros((len(keywords), Lmax), dtype=np.int32)
    for k, y in enumerate(keywords):
        kw_col[k, : len(y)] = [index[int(t)] for t in y]
    return np.asarray(cols, dtype=np.int32), kw_col, np.asarray([len(y) for y in keywords], dtype=np.int32)


class Call:
    """One oe_ctc_kws call with its device buffers: sentinel-filled outputs, run() launches on the current stream."""

    def __init__(self, logits, hlens, keywords, thr, max_hits, normalized, ldv=None, want_best=True, Lmax=None):
        logits = torch.as_tensor(np.asarray(logits), dtype=torch.float32)
        B, T, V = logits.shape
        self.ldv = ldv or V
        self.buf = torch.zeros(B, T, self.ldv, device=DEV)
        self.buf[:, :, :V] = logits.to(DEV)
        cols, kw_col, klens = tables(keywords, Lmax)
        K = len(keywords)
        self.t = [torch.from_numpy(a).to(DEV) for a in (cols, kw_col, klens, np.asarray(thr, dtype=np.float32))]
        self.hl = torch.as_tensor(np.asarray(hlens), dtype=torch.int32).to(DEV)
        self.set = hip.KeywordSet(self.t[0].data_ptr(), len(cols), self.t[1].data_ptr(), self.t[2].data_ptr(), self.t[3].data_ptr(), K,
                                  kw_col.shape[1])
        self.ws = torch.empty(max(hip.lib().oe_ctc_kws_workspace_bytes(B, T, len(cols)), 16), dtype=torch.uint8, device=DEV)
        self.shape, self.max_hits, self.want_best = (B, T, V, K), max_hits, want_best
        a = self.args = hip.CtcKwsArgs()
        a.logits, a.ldv, a.B, a.T, a.V, a.hlens = self.buf.data_ptr(), self.ldv, B, T, V, self.hl.data_ptr()
        a.kws, a.normalized, a.max_hits, a.workspace = C.pointer(self.set), int(normalized), max_hits, self.ws.data_ptr()
        self.fresh_outputs()

    def fresh_outputs(self):
        B, _, _, K = self.shape
        i32 = lambda *s: torch.full(s, SENT_I, dtype=torch.int32, device=DEV)
        f32 = lambda *s: torch.full(s, SENT_F, dtype=torch.float32, device=DEV)
        self.out = [i32(B, K), i32(B, K, self.max_hits), i32(B, K, self.max_hits), f32(B, K, self.max_hits)]
        self.out += [i32(B, K), i32(B, K), f32(B, K)] if self.want_best else [None, None, None]
        a = self.args
        a.n_hits, a.hit_start, a.hit_end, a.hit_score, a.best_start, a.best_end, a.best_score = (
            None if t is None else t.data_ptr() for t in self.out)

    def launch(self):
        return hip.lib().oe_ctc_kws(C.byref(self.args), hip.stream())

    def run(self):
        hip.check(self.launch(), "oe_ctc_kws")
        torch.cuda.synchronize()
        return self.numpy()

    def numpy(self):
        return [None if t is None else t.cpu().numpy() for t in self.out]

    def untouched(self):
        return all(bool((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all()) for t in self.out if t is not None)


def assert_equal_outputs(got, want):
    for name, g, w in zip(NAMES, got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())


# ---------------------------------------------------------------- exact mode
def labels(rng, V, L, repeat=False):
    y = [int(c) for c in rng.integers(1, V, size=L)]
    if repeat and L > 1:
        y[1] = y[0]
    return y


def exact_case(name):
    """-> dict(lp (B, T, V) float64 on the 1/8 grid, hlens, keywords, thr, max_hits, ldv, min_hits)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    c = dict(B=1, T=90, V=6, max_hits=4, ldv=None, thr=-0.5, min_hits=1, Lmax=None)
    if name == "L1":
        c.update(kw=[[1], [4], [5]], max_hits=90)
    elif name == "L2_repeated":
        c.update(kw=[[2, 2], [3, 3], [1, 2]])
    elif name == "L32":
        c.update(kw=[labels(rng, 6, 32), labels(rng, 6, 32, repeat=True)], T=400, thr=-1.0)
    elif name == "mixed_L_1_7_32_with_an_empty_keyword":
        c.update(kw=[[3], labels(rng, 6, 7), [], labels(rng, 6, 32), [2, 1]], T=300, thr=-1.0)
    elif name == "K1":
        c.update(kw=[[2, 4, 1]])
    elif name == "K5":
        c.update(kw=[labels(rng, 6, int(rng.integers(1, 5))) for _ in range(5)])
    elif name == "K9_B2":
        c.update(kw=[labels(rng, 6, int(rng.integers(1, 5))) for _ in range(9)], B=2, hlens=[90, 55])
    elif name == "hlens_0_1_T":
        c.update(kw=[[2], [1, 3], [3, 1, 2]], B=3, hlens=[0, 1, 90])
    elif name == "fewer_frames_than_labels":
        c.update(kw=[[1, 2, 3, 4, 5], [2, 2, 2], [4]], B=2, hlens=[3, 4], min_hits=0)
    elif name in ("T15", "T16", "T17"):
        c.update(kw=[[1, 2], [3], [2, 1, 3]], T=int(name[1:]), thr=-1.5, min_hits=0)
    elif name == "T5000":
        c.update(kw=[[1, 2, 3], [4, 4], labels(rng, 6, 9)], T=5000, max_hits=8, thr=-0.25)
    elif name == "ldv_wider_than_V":
        c.update(kw=[[1, 5], [5, 2, 2]], ldv=9, B=2)
    elif name == "max_hits_1":
        c.update(kw=[[1, 2], [3]], max_hits=1, T=200, min_hits=4)
    elif name == "label_outside_the_vocabulary":
        c.update(kw=[[1, 9, 2], [-2, 1], [5, 7], [9, 11, 9]], V=8)
    elif name == "shared_tokens":
        c.update(kw=[[1, 2, 3], [3, 2, 1], [2, 2, 1, 3]])
    else:
        raise KeyError(name)
    c.setdefault("hlens", [c["T"]] * c["B"])
    c["lp"] = np.stack([R.grid_case(rng, c["T"], c["V"]) for _ in range(c["B"])])
    c["thr"] = [c["thr"]] * len(c["kw"])
    return c


EXACT = ["L1", "L2_repeated", "L32", "mixed_L_1_7_32_with_an_empty_keyword", "K1", "K5", "K9_B2", "hlens_0_1_T",
         "fewer_frames_than_labels", "T15", "T16", "T17", "T5000", "ldv_wider_than_V", "max_hits_1", "label_outside_the_vocabulary",
         "shared_tokens"]


@pytest.mark.parametrize("name", EXACT)
def test_exact_mode_equals_the_restatement_bit_for_bit(name):
    c = exact_case(name)
    want = R.search(c["lp"], c["hlens"], c["kw"], c["thr"], c["max_hits"])
    call = Call(c["lp"], c["hlens"], c["kw"], c["thr"], c["max_hits"], True, ldv=c["ldv"], Lmax=c["Lmax"])
    got = call.run()
    n = want[0]
    print(f"{name}: n_hits {n.tolist()}")
    assert_equal_outputs(got, want)
    assert int(n.sum()) >= c["min_hits"]
    if name == "max_hits_1":
        assert (n > 1).any()                                 # the count exceeds the stored hits
    if name == "shared_tokens":
        assert call.set.U == 3 < sum(len(y) for y in c["kw"])
    if name == "fewer_frames_than_labels":
        assert n[:, :2].sum() == 0 and (want[4][:, :2] == -1).all() and np.isneginf(want[6][:, :2]).all()
    # the optional outputs are optional: without them the rest is the same
    bare = Call(c["lp"], c["hlens"], c["kw"], c["thr"], c["max_hits"], True, ldv=c["ldv"], want_best=False).run()
    assert_equal_outputs(bare[:4], want[:4])


# ---------------------------------------------------------------- raw mode
@functools.lru_cache(maxsize=None)
def raw_batch():
    """Two recordings (T = 600 and 300) of the continuous fixtures, their float64 candidates and hits: computed once."""
    seeds = (100, 101)
    fx = [R.raw_fixture(s) for s in seeds]
    kws = fx[0][1]
    T, V = 600, fx[0][0].shape[1]
    logits = np.zeros((2, T, V), dtype=np.float32)
    hlens = [f[0].shape[0] for f in fx]
    for b, f in enumerate(fx):
        logits[b, : hlens[b]] = f[0]
    lp = [R.log_softmax(logits[b, : hlens[b]]) for b in range(2)]
    cands = [[R.candidates(lp[b], y) for y in kws] for b in range(2)]
    ref = [[R.scan(c, LOG_HALF) for c in cands[b]] for b in range(2)]
    return logits, hlens, kws, [f[2] for f in fx], lp, cands, ref


def test_raw_mode_against_float64_optima():
    logits, hlens, kws, planted, lp, cands, ref = raw_batch()
    K = len(kws)
    n_hits, hs, he, hv, bs, be, bv = Call(logits, hlens, kws, [LOG_HALF] * K, 8, False).run()
    for b in range(2):
        Tb, total = hlens[b], 0
        for k, y in enumerate(kws):
            n = int(n_hits[b, k])
            assert 0 <= n <= 8
            total += n
            free = {t: sc for t, _, sc in cands[b][k]}
            last = -1
            for i in range(n):
                s, e, sc = int(hs[b, k, i]), int(he[b, k, i]), float(hv[b, k, i])
                assert last < s <= e < Tb, (b, k, i)                     # well-formed, disjoint, in time order
                last = e
                np.testing.assert_allclose(sc, R.span_optimum(lp[b], y, s, e), rtol=RTOL, atol=ATOL)
                np.testing.assert_allclose(sc, free[e], rtol=RTOL, atol=ATOL)
            assert (hs[b, k, n:] == -1).all() and (he[b, k, n:] == -1).all() and (hv[b, k, n:] == 0).all()
            got = [(int(hs[b, k, i]), int(he[b, k, i])) for i in range(n)]
            hits64, best64 = ref[b][k]
            for s, e, sc in hits64:
                m = e - s + 1
                if sc >= (LOG_HALF + 1e-3) * m + 1e-3:                   # clears the threshold by more than the tolerance
                    assert any(gs <= e and s <= ge for gs, ge in got), (b, k, s, e, got)
            np.testing.assert_allclose(bv[b, k], best64[2], rtol=RTOL, atol=ATOL)
            assert 0 <= bs[b, k] <= be[b, k] < Tb
            for kk, s, e in planted[b]:
                if kk == k:
                    assert (s, e) in got, (b, k, s, e, got)
        print(f"recording {b}: {total} hits in {Tb} frames, {len(planted[b])} planted")
        assert len(planted[b]) >= 3 and 3 <= total < Tb                  # not vacuous


# ---------------------------------------------------------------- error paths
@pytest.mark.parametrize("what,text", [("K", b"K=0"), ("Lmax", b"Lmax=33"), ("U", b"U=6"), ("hlens", b"hlens")])
def test_bad_arguments_leave_the_outputs_untouched(what, text):
    c = exact_case("K1")
    call = Call(c["lp"], c["hlens"], c["kw"], c["thr"], 4, True)
    if what == "K":
        call.set.K = 0
    elif what == "Lmax":
        call.set.Lmax = 33
    elif what == "U":
        call.set.U = c["V"]
    else:
        call.args.hlens = None
    lib = hip.lib()
    rc = call.launch()
    assert rc != 0 and text in lib.oe_last_error(), lib.oe_last_error()
    torch.cuda.synchronize()
    assert call.untouched()


# ---------------------------------------------------------------- capture
def test_captured_in_a_graph_replays_identically():
    c = exact_case("K5")
    want = R.search(c["lp"], c["hlens"], c["kw"], c["thr"], c["max_hits"])
    call = Call(c["lp"], c["hlens"], c["kw"], c["thr"], c["max_hits"], True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.check(call.launch(), "oe_ctc_kws")
        torch.cuda.synchronize()
        call.fresh_outputs()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            hip.check(call.launch(), "oe_ctc_kws")
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    seen = []
    for _ in range(2):
        for t in call.out:                                                # fresh sentinels in the buffers the graph writes
            t.fill_(SENT_I if t.dtype == torch.int32 else SENT_F)
        torch.cuda.synchronize()
        assert call.untouched()
        g.replay()
        torch.cuda.synchronize()
        seen.append(call.numpy())
        assert_equal_outputs(seen[-1], want)
    assert_equal_outputs(seen[0], seen[1])


# ---------------------------------------------------------------- python layers
def test_ops_keyword_groups_equal_the_one_call_result():
    from openeat_amd import ops
    from openeat_amd.utils.keyword import KeywordList
    logits, hlens, kws, planted, _, _, ref = raw_batch()
    kl = KeywordList(kws, threshold=0.5)
    U, (B, T, V) = len(kl.cols), logits.shape
    assert U == 39
    lg, hl = torch.from_numpy(logits).to(DEV), torch.tensor(hlens, device=DEV)
    whole = ops.ctc_keyword_search(lg, hl, kl, max_hits=8)
    cap = B * T * 4 * (35 + 1)                                            # 35 of the 39 distinct tokens a group
    bounds = kl.group_bounds(35)
    assert len(bounds) == 4, bounds                                       # three groups
    parts = ops.ctc_keyword_search(lg, hl, kl, max_hits=8, max_workspace_bytes=cap)
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, whole, parts):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert int(whole[0].sum()) >= 6
    direct = Call(logits, hlens, kws, kl.log_thr, 8, False).run()
    assert_equal_outputs([t.cpu().numpy() for t in whole], direct)
    with pytest.raises(TypeError):
        ops.ctc_keyword_search(lg, hl, kws)


def greedy_runs(frames):
    """[(token, first frame, last frame)] of the non-blank runs of a greedy frame path."""
    runs, prev = [], None
    for t, c in enumerate(frames):
        if c != prev and c != 0:
            runs.append([c, t, t])
        elif c != 0:
            runs[-1][2] = t
        prev = c
    return runs


def test_model_keyword_search_finds_the_greedy_ngrams():
    from openeat_amd.models.asr_model import ASRModel
    from openeat_amd.utils.align import frame_times
    from openeat_amd.utils.keyword import KeywordList
    torch.manual_seed(11)
    V = 12
    model = ASRModel(80, V, encoder_num_blocks=2, decoder_num_blocks=1, d_model=64, attention_heads=4, linear_units=128,
                     dropout_rate=0.0)
    with torch.no_grad():                                                 # sharp posteriors: the greedy path stands out
        model.ctc.ctc_lo.weight.mul_(30.0)
    model = model.to(DEV).eval()
    feats = torch.randn(2, 140, 80, generator=torch.Generator().manual_seed(12)).to(DEV)
    flen = torch.tensor([140, 101], device=DEV)
    with torch.no_grad():
        enc, mask, _ = model._encode(feats, flen)
        lens = mask.squeeze(1).sum(1).tolist()
        fb = model.ctc.argmax(enc).cpu().tolist()
    runs = [greedy_runs(fb[b][: lens[b]]) for b in range(2)]
    assert all(len(r) >= 3 for r in runs), runs
    grams = []
    for r in runs:
        toks = [c for c, _, _ in r]
        for n in (1, 2, 3):
            for i in range(len(toks) - n + 1):
                if tuple(toks[i:i + n]) not in grams:
                    grams.append(tuple(toks[i:i + n]))
    grams = grams[:40]
    kl = KeywordList(grams, threshold=1e-6)
    hits, truncated = model.keyword_search(feats, flen, kl, max_hits=64, with_times=True)
    assert len(hits) == 2 and len(truncated) == 2 and all(len(f) == len(grams) for f in truncated)
    rate = model.encoder.embed.subsampling_rate
    found = 0
    for b in range(2):
        assert not any(truncated[b])
        starts = [h["start_frame"] for h in hits[b]]
        assert starts == sorted(starts)                                   # time order
        for h in hits[b]:
            assert set(h) == {"keyword", "tokens", "start_frame", "end_frame", "score", "confidence", "start_s", "end_s"}
            n = h["end_frame"] - h["start_frame"] + 1
            assert 0 <= h["start_frame"] <= h["end_frame"] < lens[b] and h["tokens"] == list(grams[h["keyword"]])
            assert h["confidence"] == math.exp(h["score"] / n) and 1e-6 <= h["confidence"] <= 1.0
            assert (h["start_s"], h["end_s"]) == frame_times(h["start_frame"], h["end_frame"], rate)
        toks = [c for c, _, _ in runs[b]]
        for k, g in enumerate(grams):
            for i in range(len(toks) - len(g) + 1):
                if tuple(toks[i:i + len(g)]) == g:                       # the greedy path emits g on frames f0 .. f1
                    f0, f1 = runs[b][i][1], runs[b][i + len(g) - 1][2]
                    inside = [h for h in hits[b] if h["keyword"] == k and f0 <= h["start_frame"] and h["end_frame"] <= f1]
                    assert inside, (b, g, f0, f1, [(h["start_frame"], h["end_frame"]) for h in hits[b] if h["keyword"] == k])
                    found += 1
    assert found >= len(grams)
    plain, _ = model.keyword_search(feats, flen, kl, max_hits=64)
    assert [[{k: v for k, v in h.items() if not k.endswith("_s")} for h in rec] for rec in hits] == plain
    few, trunc1 = model.keyword_search(feats, flen, kl, max_hits=1)
    assert all(sum(h["keyword"] == k for h in few[b]) <= 1 for b in range(2) for k in range(len(grams)))
    many = [[sum(h["keyword"] == k for h in hits[b]) > 1 for k in range(len(grams))] for b in range(2)]
    assert trunc1 == many
    with pytest.raises(ValueError):
        model.keyword_search(feats, flen, [list(g) for g in grams])


def test_model_keyword_search_over_windowed_logits():
    """The shapes of test_ctc_segment_gpu.py: a window of the whole recording gives the plain pass's logits exactly, hence the
    same hits; windows of 8 frames with a margin of 4 give the windows' own rows, hence hits of the same form."""
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    from openeat_amd.utils.keyword import KeywordList
    from openeat_amd.utils.segment import encoder_frames
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    feats, flen = g["in"]["feats"], g["in"]["flen"]
    rec = torch.cat([feats[b, : int(flen[b])] for b in range(feats.shape[0])])[None].to(DEV)
    model, n = model.to(DEV).eval(), torch.tensor([rec.shape[1]], device=DEV)
    embed = model.encoder.embed
    n_enc = encoder_frames(int(n[0]), embed.subsampling_rate, embed.right_context)
    with torch.no_grad():
        enc, _, _ = model._encode(rec, n)
        runs = greedy_runs(model.ctc.argmax(enc)[0].cpu().tolist())
    toks = [c for c, _, _ in runs]
    assert len(toks) >= 3
    grams = list(dict.fromkeys([(c,) for c in toks] + [tuple(toks[i:i + 2]) for i in range(len(toks) - 1)]))
    kl = KeywordList(grams, threshold=1e-6)
    plain, tr0 = model.keyword_search(rec, n, kl, max_hits=32)
    whole, tr1 = model.keyword_search(rec, n, kl, window=n_enc, margin=4, max_hits=32)
    assert plain == whole and tr0 == tr1 and len(plain[0]) >= 3
    assert 8 < n_enc
    win, _ = model.keyword_search(rec, n, kl, window=8, margin=4, max_hits=32)
    assert len(win) == 1 and len(win[0]) >= 1
    for h in win[0]:
        assert set(h) == set(plain[0][0]) and 0 <= h["start_frame"] <= h["end_frame"] < n_enc
