"""GPU: CTC prefix beam search with n-gram LM shallow fusion on the device (oe_ctc_prefix_beam with an LM) against the yardstick
(tests/ctc_lm_beam_ref.py: the reference's dict loop with the fused key, RefLM for the LM terms - independent of the product
and held to the host recursion and to RefLM.score by tests/test_ctc_lm_beam_ref.py), run on the device's own top-k.

Bounds: the same prefixes in the same order, exactly (the cases keep neighbouring totals 1e-8 apart or exactly equal, which
the yardstick reports and this file asserts again on the top-k it really used); total and ctc within 1e-9 * max(1, |x|)
(device exp / log, as the plain device-beam test allows); lm within 2**-52 * n * S, n float32 values of summed magnitude S
(both sides add the same float32 values in float64), the bound of tests/test_ngram_gpu.py."""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_lm_beam_ref as R  # noqa: E402
import ngram_ref  # noqa: E402
from conftest import load_golden, load_golden_json  # noqa: E402
from openeat_amd.models.asr_model import ASRModel  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402

DEV = "cuda"
GAP_FLOOR = 1e-8
NEG = -np.inf


def _close(a, b):
    return a == b or abs(a - b) <= 1e-9 * max(1.0, abs(b))


def _compare(got, want, ref, t2c, eos, where):
    """One utterance: device n-best [(prefix, total, ctc, lm)] against the yardstick's."""
    assert [h[0] for h in got] == [h[0] for h in want], (where, got[:3], want[:3])
    for g, w in zip(got, want):
        assert _close(g[1], w[1]) and _close(g[2], w[2]), (where, g, w)
        _, n, S = ref.score(" ".join(t2c[t] for t in g[0]), bos=True, eos=eos)
        assert abs(g[3] - w[3]) <= 2.0 ** -52 * n * S, (where, g, w)


def _lists(raw, B, beam):
    pre, plen, total, ctc, lms, bad = [x.cpu().numpy() for x in raw]
    assert int(bad[0]) == 0
    return [[(tuple(pre[b, i, : plen[b, i]].tolist()), float(total[b, i]), float(ctc[b, i]), float(lms[b, i]))
             for i in range(beam) if plen[b, i] >= 0] for b in range(B)]


def _check_missing(raw, n_real):
    """Slots behind the n_real[b] prefixes that exist: length -1, scores -inf - and no others."""
    _, plen, total, ctc, lms, _ = [x.cpu().numpy() for x in raw]
    for b, n in enumerate(n_real):
        assert (plen[b, :n] >= 0).all() and (plen[b, n:] == -1).all(), (b, plen[b])
        for x in (total, ctc, lms):
            assert np.isfinite(x[b, :n]).all() and (x[b, n:] == NEG).all(), (b, x[b])


@pytest.mark.parametrize("B,T,V,beam,sharp,order", R.CASES)
def test_fused_beam_equals_the_yardstick(tmp_path, B, T, V, beam, sharp, order):
    from openeat_amd import hip, ops
    logits, lens, path, t2c = R.make_case(tmp_path, B, T, V, beam, sharp, order)
    ref = ngram_ref.RefLM(path)
    lm = NgramLM(path, t2c)
    assert lm.order == order
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    dlens = lens.to(DEV)
    plm = R.PrefixLM(ref, t2c)
    plain = hip.ctc_prefix_beam_device(top_p, top_i, dlens, beam)
    for lw, lb in R.WEIGHTS:
        for eos in (True, False):
            where = (lw, lb, eos)
            raw = hip.ctc_prefix_beam_lm_device(top_p, top_i, dlens, beam, lm, lw, lb, eos, raw=True)
            torch.cuda.synchronize()
            got = _lists(raw, B, beam)
            gaps = []
            for b in range(B):
                want, gap = R.search(hp[b, : lens[b]], hi[b, : lens[b]], beam, plm, lw, lb, eos)
                gaps.append(gap)
                assert gap >= GAP_FLOOR, (where, b, gap)                    # the case is decidable on this top-k too
                _compare(got[b], want, ref, t2c, eos, where + (b,))
            _check_missing(raw, [len(u) for u in got])
            print(f"weights ({lw}, {lb}) eos {eos}: smallest non-zero gap {min(gaps):.3g}")
            # the list form returns the same
            assert hip.ctc_prefix_beam_lm_device(top_p, top_i, dlens, beam, lm, lw, lb, eos) == got
            # LM column against the scoring kernel, on the device
            pre, plen, _, _, lms, _ = raw
            s = ops.ngram_score(lm, pre.view(B * beam, -1), plen.view(-1), bos=True, eos=eos).view(B, beam).cpu().numpy()
            lms = lms.cpu().numpy()
            for b in range(B):
                for i in range(beam):
                    if i >= len(got[b]):
                        assert s[b, i] == NEG and lms[b, i] == NEG
                        continue
                    _, n, S = ref.score(" ".join(t2c[t] for t in got[b][i][0]), bos=True, eos=eos)
                    assert abs(s[b, i] - lms[b, i]) <= 2.0 ** -52 * n * S, (where, b, i, s[b, i], lms[b, i])
            if (lw, lb) == (0.0, 0.0):                                      # zero weights: the plain device search, bit for bit
                for b in range(B):
                    assert [h[0] for h in got[b]] == [p for p, _ in plain[b]], (where, b)
                    a = np.array([h[2] for h in got[b]]).view(np.int64)
                    assert np.array_equal(a, np.array([s_ for _, s_ in plain[b]]).view(np.int64)), (where, b)
    if (B, T, V) == R.CASES[0][:3]:                                         # the zero-frame utterance: the one empty prefix
        assert [h[0] for h in got[1]] == [()]
    # no lengths given: every utterance uses all T frames
    got_all = hip.ctc_prefix_beam_lm_device(top_p, top_i, None, beam, lm, 0.5, 0.0, True)
    for b in range(B):
        want, _ = R.search(hp[b], hi[b], beam, plm, 0.5, 0.0, True)
        assert [h[0] for h in got_all[b]] == [h[0] for h in want], b


def test_exact_ties_under_fusion_keep_insertion_order(tmp_path):
    """Uniform frames and an LM in which every word costs exactly -1: three prefixes share the best total (a CPU test shows
    it); the device resolves every tie as the dict loop's stable sort does."""
    from openeat_amd import hip, ops
    logits, lens, path, t2c, beam = R.tie_case(tmp_path)
    ref = ngram_ref.RefLM(path)
    lm = NgramLM(path, t2c)
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    plm = R.PrefixLM(ref, t2c)
    for lw, lb in ((0.5, 0.0), (0.5, 1.0)):
        got = hip.ctc_prefix_beam_lm_device(top_p, top_i, lens.to(DEV), beam, lm, lw, lb, True)
        for b in range(logits.shape[0]):
            want, gap = R.search(hp[b, : lens[b]], hi[b, : lens[b]], beam, plm, lw, lb, True)
            assert gap >= GAP_FLOOR
            if b == 0:
                assert want[0][1] == want[1][1] == want[2][1]
            _compare(got[b], want, ref, t2c, True, (lw, lb, b))


def test_one_capture_replayed_twice_gives_the_eager_bits(tmp_path):
    from openeat_amd import hip, ops
    B, T, V, beam, sharp, order = R.CASES[0]
    logits, lens, path, t2c = R.make_case(tmp_path, B, T, V, beam, sharp, order)
    lm = NgramLM(path, t2c)
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    dlens = lens.to(DEV)
    eager = [x.clone() for x in hip.ctc_prefix_beam_lm_device(top_p, top_i, dlens, beam, lm, 0.3, 0.8, True, raw=True)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.ctc_prefix_beam_lm_device(top_p, top_i, dlens, beam, lm, 0.3, 0.8, True, raw=True)
    for _ in range(2):
        for x in out[:5]:
            x.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        plen = eager[1]
        assert torch.equal(out[1], plen) and int(out[5][0]) == 0
        for e, o in zip(eager[2:5], out[2:5]):
            assert torch.equal(e.view(torch.int64), o.view(torch.int64))
        pos = torch.arange(eager[0].shape[2], device=DEV).view(1, 1, -1)
        used = pos < plen.unsqueeze(2)
        assert torch.equal(eager[0][used], out[0][used])


def test_bad_arguments_are_reported_not_launched(tmp_path):
    from openeat_amd import hip
    path = str(tmp_path / "s.arpa")
    words = ngram_ref.random_arpa(path, 2, 10, 30, np.random.default_rng(1))
    lm = NgramLM(path, ["<blank>"] + words)
    B, T = 2, 6
    top_p = torch.zeros(B, T, 17, device=DEV)
    top_i = torch.zeros(B, T, 17, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="beam must be 1..16"):
        hip.ctc_prefix_beam_lm_device(top_p, top_i, None, 17, lm, 0.5)
    ws = torch.zeros(B * T * 4 * 2 + 1, dtype=torch.int32, device=DEV)
    pre = torch.zeros(B, 4, T, dtype=torch.int32, device=DEV)
    plen = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    sc = [torch.zeros(B, 4, dtype=torch.float64, device=DEV) for _ in range(3)]

    def call(**model_fields):
        model = hip.ngram_model(lm, DEV)
        for k, v in model_fields.items():
            setattr(model, k, v)
        hip.prefix_beam(hip.prefix_beam_args(top_p, top_i, None, 4, T, ws, pre, plen, *sc, lm=model, lm_weight=0.5, length_bonus=0.0, eos=True))

    with pytest.raises(RuntimeError, match="order must be 1..5"):
        call(order=6)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(table=None)
    torch.cuda.synchronize()
    assert int(plen.abs().sum()) == 0 and all(float(x.abs().sum()) == 0.0 for x in sc)      # nothing ran


# ------------------------------------------------------------------ through the model ---------------------------------
def _model():
    g = load_golden("f12_tiny_conformer")
    meta = load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), meta["V"]


def _built_lm(tmp_path, V, seed):
    """A normalised 3-gram LM over the strings str(t), as tests/test_ngram_gpu.py builds one: the alternation language the
    untrained golden model emits, with an opinion about sentence ends, beside random sentences that give every token a count."""
    rng = np.random.default_rng(seed)
    vocab = [str(t) for t in range(V)]
    corpus = [["9", "35"] * int(rng.integers(2, 9)) for _ in range(600)]
    corpus += [[vocab[i] for i in rng.integers(0, V, int(rng.integers(1, 14)))] for _ in range(300)]
    path = str(tmp_path / f"lm{seed}.arpa")
    ngram_ref.build_arpa(path, corpus, 3, vocab)
    return NgramLM(path, vocab), ngram_ref.RefLM(path), vocab


def _ragged(seed, lens):
    feats = torch.randn(len(lens), max(lens), 80, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        feats[b, n:] = 0.0
    return feats.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


def test_model_ctc_lm_beam_search_equals_the_yardstick(tmp_path):
    from openeat_amd import ops
    model, V = _model()
    lm, ref, t2c = _built_lm(tmp_path, V, 51)
    feats, flen = _ragged(37, [97, 83, 64, 41, 23])
    beam, lw, lb = 4, 0.5, 0.2
    got = model.ctc_lm_beam_search(feats, flen, beam, lm, lw, lb)
    with torch.no_grad():
        encoder_out, encoder_mask, _ = model._encode(feats, flen)
        lens = encoder_mask.squeeze(1).sum(1).cpu().tolist()
        top_p, top_i = ops.topk_rows(model.ctc.logits(encoder_out), beam, log_softmax=True)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    plm = R.PrefixLM(ref, t2c)
    for b in range(len(lens)):
        want, gap = R.search(hp[b, : lens[b]], hi[b, : lens[b]], beam, plm, lw, lb, True)
        print(f"utterance {b}: {lens[b]} frames, smallest non-zero gap {gap:.3g}")
        _compare(got[b], want, ref, t2c, True, b)
    for bad in (dict(lm=None), dict(beam_size=17)):
        kw = dict(beam_size=beam, lm=lm)
        kw.update(bad)
        with pytest.raises(ValueError):
            model.ctc_lm_beam_search(feats, flen, kw["beam_size"], kw["lm"], lw)


def test_rescoring_with_first_pass_lm(tmp_path, monkeypatch):
    """attention_rescoring_batch(first_pass_lm=True): eager, first sight under graphs and replay return the same tokens, each
    of them a member of the fused n-best; with the flag off the call is the one without the new parameters."""
    from openeat_amd.models import asr_model
    model, V = _model()
    lm, _, _ = _built_lm(tmp_path, V, 51)
    feats, flen = _ragged(41, [97, 83, 64, 41, 23])
    beam = 4
    kw = dict(ctc_weight=0.5, reverse_weight=0.3, lm=lm, lm_weight=3.0)
    fp = dict(first_pass_lm=True, first_pass_lm_weight=0.7, length_bonus=0.4)
    with torch.no_grad():
        eager = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, **kw, **fp)
        first = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, **kw, **fp)
        replay = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, **kw, **fp)
        nbest = model.ctc_lm_beam_search(feats, flen, beam, lm, 0.7, 0.4)
        off = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, first_pass_lm=False, first_pass_lm_weight=0.7,
                                              length_bonus=0.4, **kw)
        parent = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, **kw)
        off_g = model.attention_rescoring_batch(feats, flen, beam, use_graphs=True, first_pass_lm=False, **kw)
        default_w = model.attention_rescoring_batch(feats, flen, beam, use_graphs=False, first_pass_lm=True, **kw)
        nbest_w = model.ctc_lm_beam_search(feats, flen, beam, lm, 3.0)
    assert first == eager and replay == eager
    for b, h in enumerate(eager):
        assert tuple(h) in {p for p, _, _, _ in nbest[b]}, (b, h)
    for b, h in enumerate(default_w):                                     # the first-pass weight defaults to lm_weight
        assert tuple(h) in {p for p, _, _, _ in nbest_w[b]}, (b, h)
    assert off == parent and off_g == parent
    specs = [k[2] for k in model._decode_graphs if k[0] == "s1"]
    assert any(s.plain for s in specs)
    assert any(s.lm is lm and s.context is None and (s.lm_weight, s.length_bonus, s.eos) == (0.7, 0.4, True) for s in specs)
    with pytest.raises(ValueError):
        model.attention_rescoring_batch(feats, flen, 17, **kw, **fp)
    monkeypatch.setattr(asr_model, "DEVICE_BEAM", False)
    with pytest.raises(ValueError):
        model.attention_rescoring_batch(feats, flen, beam, **kw, **fp)
    alive = weakref.ref(lm)                                                 # the key holds the LM itself: the tables a cached capture
    del lm, kw, specs                                                       # points at outlive the caller's reference
    gc.collect()
    assert any(k[0] == "s1" and k[2].lm is alive() is not None for k in model._decode_graphs)
