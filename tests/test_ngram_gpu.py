"""GPU: n-gram LM scoring on the device - oe_ngram_score through the C ABI against the yardstick (tests/ngram_ref.py: the ARPA
back-off definition as a dict and a recursion, independent of the product), and the LM term of attention_rescoring_batch
against the one-utterance API, which scores on the host with NgramLM.score (held to the same yardstick by the CPU tests).

Bounds: matched orders exactly; values within 2**-52 * n * S, n = how many float32 values the yardstick summed for the
sentence and S the sum of their magnitudes - both sides add the same float32 values in float64, only the order differs."""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ngram_ref  # noqa: E402
from conftest import load_golden, load_golden_json  # noqa: E402
from openeat_amd.models.asr_model import ASRModel  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402

DEV = "cuda"
LENGTHS = [0, 1, 63, 64, 65, 248, 398]
FILL_LP, FILL_ORDER = 7.5, -7


def _stress_model(tmp_path, order, rng, with_unk):
    """A random ARPA of ~200 k n-grams over 1000 words; 900 tokens: 800 of its words and 100 strings it does not list."""
    path = str(tmp_path / f"stress{order}.arpa")
    per = 200_000 // max(order - 1, 1)
    words = ngram_ref.random_arpa(path, order, 1000, per, rng, with_unk=with_unk)
    t2c = [words[i] for i in rng.permutation(1000)[:800]] + [f"oov{i}" for i in range(100)]
    t2c = [t2c[i] for i in rng.permutation(900)]
    return path, t2c


def _hypotheses(ref, t2c, R, ld, rng):
    """Token rows of the wanted lengths: half random tokens, half walks along LISTED n-grams of every order (so that the
    longer matches really occur); some slots missing (negative length); garbage - not padding ids - behind every length."""
    tok_of = {s: i for i, s in enumerate(t2c)}
    listed = [[g for g in ref.grams if len(g) == k and all(w in tok_of for w in g)] for k in range(1, ref.order + 1)]
    lens = np.array([LENGTHS[r % len(LENGTHS)] if r < 4 * len(LENGTHS) else int(rng.integers(0, 120)) for r in range(R)], dtype=np.int32)
    tokens = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(R, ld), dtype=np.int64).astype(np.int32)
    for r in range(R):
        row = []
        while len(row) < lens[r]:
            if rng.random() < 0.5:
                row.append(int(rng.integers(0, len(t2c))))
            else:
                k = int(rng.integers(0, ref.order))
                if listed[k]:
                    row.extend(tok_of[w] for w in listed[k][int(rng.integers(0, len(listed[k])))])
        tokens[r, : lens[r]] = row[: lens[r]]
    missing = rng.random(R) < 0.08
    missing[: 2 * len(LENGTHS)] = False
    klens = np.where(missing, -1 - rng.integers(0, 5, R), lens).astype(np.int32)
    return tokens, lens, klens


def _call(lm, tokens, klens, bos, eos):
    from openeat_amd import hip
    R, ld = tokens.shape
    tk = torch.from_numpy(tokens).to(DEV)
    kl = torch.from_numpy(klens).to(DEV)
    score = torch.full((R,), 123.0, dtype=torch.float64, device=DEV)
    tok_logp = torch.full((R, ld + 1), FILL_LP, dtype=torch.float64, device=DEV)
    tok_order = torch.full((R, ld + 1), FILL_ORDER, dtype=torch.int32, device=DEV)
    hip.call("oe_ngram_score", hip.ngram_model(lm, DEV), tk, ld, kl, R, int(bos), int(eos), score, tok_logp, tok_order)
    torch.cuda.synchronize()
    return score.cpu().numpy(), tok_logp.cpu().numpy(), tok_order.cpu().numpy()


def _check(ref, t2c, tokens, lens, klens, bos, eos, got, rows):
    score, tok_logp, tok_order = got
    worst = 0.0
    for r in rows:
        if klens[r] < 0:
            assert score[r] == -np.inf, r
            assert (tok_logp[r] == FILL_LP).all() and (tok_order[r] == FILL_ORDER).all(), r
            continue
        n_out = int(lens[r]) + (1 if eos else 0)
        want, n, S = ref.full_scores(" ".join(t2c[t] for t in tokens[r, : lens[r]]), bos, eos)
        assert len(want) == n_out
        tol = 2.0 ** -52 * n * S
        assert tok_order[r, :n_out].tolist() == [o for _, o, _ in want], (r, int(lens[r]))
        err = max([abs(tok_logp[r, j] - want[j][0]) for j in range(n_out)] + [abs(score[r] - sum(v for v, _, _ in want))])
        assert err <= tol, (r, int(lens[r]), err, tol)
        worst = max(worst, err / tol if tol > 0 else 0.0)
        assert (tok_logp[r, n_out:] == FILL_LP).all() and (tok_order[r, n_out:] == FILL_ORDER).all(), r
    return worst


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_ngram_score_kernel_against_the_yardstick(tmp_path, order):
    rng = np.random.default_rng(700 + order)
    with_unk = order % 2 == 1
    path, t2c = _stress_model(tmp_path, order, rng, with_unk)
    ref = ngram_ref.RefLM(path)
    lm = NgramLM(path, t2c)
    assert lm.order == order and (order == 1 or lm.n_ngrams > 100_000)
    R, ld = 640, 398 + 9
    tokens, lens, klens = _hypotheses(ref, t2c, R, ld, rng)
    assert (klens < 0).any()
    got = _call(lm, tokens, klens, True, True)
    worst = _check(ref, t2c, tokens, lens, klens, True, True, got, range(R))
    orders_seen = set(np.unique(got[2][got[2] != FILL_ORDER]).tolist())
    print(f"order {order}: {lm.n_ngrams} n-grams, capacity {lm.capacity}, max_probe {lm.max_probe}, worst err/tol {worst:.3g}, "
          f"matched orders {sorted(orders_seen)}")
    assert orders_seen == set(range(1, order + 1))                      # every match length occurred
    for bos, eos in ((False, True), (True, False), (False, False)):
        got = _call(lm, tokens[:96], klens[:96], bos, eos)
        _check(ref, t2c, tokens, lens, klens, bos, eos, got, range(96))
    # the same through ops.ngram_score (int64 tokens, as the model passes them): equal bits
    from openeat_amd import ops
    s2, lp2, o2 = ops.ngram_score(lm, torch.from_numpy(tokens[:96]).to(DEV).long(), torch.from_numpy(klens[:96]).to(DEV).long(),
                                  bos=False, eos=False, per_token=True)
    assert np.array_equal(s2.cpu().numpy(), got[0])
    keep = got[2] != FILL_ORDER
    assert np.array_equal(o2.cpu().numpy()[keep], got[2][keep]) and np.array_equal(lp2.cpu().numpy()[keep], got[1][keep])


def test_two_calls_give_identical_bits(tmp_path):
    rng = np.random.default_rng(77)
    path, t2c = _stress_model(tmp_path, 3, rng, True)
    ref, lm = ngram_ref.RefLM(path), NgramLM(path, t2c)
    tokens, lens, klens = _hypotheses(ref, t2c, 640, 398, rng)
    a = _call(lm, tokens, klens, True, True)
    b = _call(lm, tokens, klens, True, True)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64))
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64)) and np.array_equal(a[2], b[2])


def test_ops_ngram_score_refuses_cpu_tensors(tmp_path):
    from openeat_amd import ops
    path = str(tmp_path / "s.arpa")
    words = ngram_ref.random_arpa(path, 2, 10, 30, np.random.default_rng(1))
    lm = NgramLM(path, words)
    with pytest.raises(TypeError):
        ops.ngram_score(lm, torch.zeros(2, 3, dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.ngram_score(lm, torch.zeros(2, 3, dtype=torch.int32, device=DEV), torch.tensor([3, 3], dtype=torch.int32))


# ------------------------------------------------------------------ through the model ---------------------------------
@pytest.fixture(params=[0, 6, 60, 62, 3], ids=["fp32-mfma", "bf16x6-mfma", "bf16x6-planes-forced", "bf16x6-fused-ffn", "bf16x3-mfma"])
def gemm_precision(request):
    """The arithmetic modes the rescoring tests of test_gpu_model.py run in (its autouse fixture is local to that file)."""
    from openeat_amd import hip, ops, planes
    old, old_min, old_pol = hip.GEMM_PRECISION, planes.MIN_SPLIT_ELEMS, planes.POLICY
    old_ffn = (ops.FUSED_FFN_MIN_ROWS, ops.FUSED_FFN_BWD)
    hip.GEMM_PRECISION = 6 if request.param in (60, 62) else request.param
    if request.param == 60:
        planes.MIN_SPLIT_ELEMS, planes.POLICY = 0, "all"
        hip.lib().oe_gemm_pl_config(0, -1, -1, -1)
    if request.param == 62:
        ops.FUSED_FFN_MIN_ROWS, ops.FUSED_FFN_BWD = 0, True
    planes.clear()
    yield request.param
    hip.GEMM_PRECISION, planes.MIN_SPLIT_ELEMS, planes.POLICY = old, old_min, old_pol
    ops.FUSED_FFN_MIN_ROWS, ops.FUSED_FFN_BWD = old_ffn
    hip.lib().oe_gemm_pl_config(96, 0, 0, 8)
    planes.clear()


LM_WEIGHT = 3.0


def _model():
    g = load_golden("f12_tiny_conformer")
    meta = load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), meta["V"]


def _built_lm(tmp_path, V, seed, tail=()):
    """A normalised 3-gram LM over the strings str(t).  The untrained golden model emits alternations "9 35 9 35 .." and its
    n-best lists are such alternations of different lengths, of which lm=None always picks the shortest (every term of the
    score is a negative log-probability).  So the corpus is that language with an opinion about where a sentence may END:
    600 sentences (9 35) x k followed by `tail` - () ends them after 35, ("9",) after 9 - beside 300 random ones that give
    every token a count.  An LM of weight 3 then prefers a hypothesis with the right ending to a shorter one with the wrong
    one, by 7 or more in the total score on this model (far above what separates the arithmetic modes)."""
    rng = np.random.default_rng(seed)
    vocab = [str(t) for t in range(V)]
    corpus = [["9", "35"] * int(rng.integers(2, 9)) + list(tail) for _ in range(600)]
    corpus += [[vocab[i] for i in rng.integers(0, V, int(rng.integers(1, 14)))] for _ in range(300)]
    path = str(tmp_path / f"lm{seed}.arpa")
    ngram_ref.build_arpa(path, corpus, 3, vocab)
    tok2chr = {t: str(t) for t in range(V)}
    return NgramLM(path, tok2chr), tok2chr


def _ragged(seed, lens):
    feats = torch.randn(len(lens), max(lens), 80, generator=torch.Generator().manual_seed(seed))      # host generator: the same
    for b, n in enumerate(lens):                                                                       # inputs on every machine
        feats[b, n:] = 0.0
    return feats.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)


def test_batched_rescoring_with_ngram_lm_equals_per_utterance_rescoring(tmp_path, gemm_precision):
    """attention_rescoring_batch(lm=NgramLM) on a ragged batch == attention_rescoring (batch of one, the LM scored on the host by
    NgramLM.score with the same token2char) on each utterance padded to 4c+3 frames - the rule of
    test_batched_rescoring_on_ragged_batch_equals_per_utterance_rescoring - and the LM term is live: for at least one utterance
    the pick differs from the lm=None pick."""
    model, V = _model()
    lm, tok2chr = _built_lm(tmp_path, V, 51)
    lens = [97, 83, 64, 41, 23, 90, 71, 55]
    feats, flen = _ragged(37, lens)
    from openeat_amd.utils.mask import make_pad_mask
    enc_frames = (~make_pad_mask(flen.cpu(), max(lens))).unsqueeze(1)[:, :, :-2:2][:, :, :-2:2].sum(-1).view(-1).tolist()
    with torch.no_grad():
        batch = model.attention_rescoring_batch(feats, flen, 4, ctc_weight=0.5, reverse_weight=0.3, lm=lm, lm_weight=LM_WEIGHT)
        plain = model.attention_rescoring_batch(feats, flen, 4, ctc_weight=0.5, reverse_weight=0.3)
        single = []
        for b, (n, c) in enumerate(zip(lens, enc_frames)):
            m = 4 * c + 3
            x = torch.zeros(1, m, 80, device=DEV)
            x[0, : min(n, m)] = feats[b, : min(n, m)]
            ml = torch.tensor([m], dtype=torch.int32, device=DEV)
            single.append(list(model.attention_rescoring(x, ml, 4, ctc_weight=0.5, reverse_weight=0.3, lm=lm, lm_weight=LM_WEIGHT,
                                                         token2char=tok2chr)[0]))
    print(f"mode {gemm_precision}: picks that differ from lm=None: {sum(a != b for a, b in zip(batch, plain))} of {len(lens)}")
    assert batch == single
    assert any(a != b for a, b in zip(batch, plain))                   # the LM term changed a pick


def test_ngram_rescoring_from_graphs_and_host_beam_equal_eager(tmp_path, gemm_precision, monkeypatch):
    """use_graphs=True == eager on first sight of a shape and on replay, also after a second NgramLM was built and used in
    between (a replay reads its own model's tables), and the host-beam route gives the same picks."""
    from openeat_amd.models import asr_model
    model, V = _model()
    lm_a, _ = _built_lm(tmp_path, V, 51)
    cases = [_ragged(41, [97, 83, 64, 41, 23]), _ragged(42, [97, 97, 97, 97, 97]), _ragged(43, [50, 97, 30, 88, 61])]
    kw = dict(ctc_weight=0.5, reverse_weight=0.3, lm_weight=LM_WEIGHT)
    with torch.no_grad():
        want_a = [model.attention_rescoring_batch(f, l, 4, lm=lm_a, use_graphs=False, **kw) for f, l in cases]
        first_a = [model.attention_rescoring_batch(f, l, 4, lm=lm_a, use_graphs=True, **kw) for f, l in cases]
        lm_b, _ = _built_lm(tmp_path, V, 52, tail=("9",))
        want_b = [model.attention_rescoring_batch(f, l, 4, lm=lm_b, use_graphs=False, **kw) for f, l in cases]
        first_b = [model.attention_rescoring_batch(f, l, 4, lm=lm_b, use_graphs=True, **kw) for f, l in cases]
        replay_a = [model.attention_rescoring_batch(f, l, 4, lm=lm_a, use_graphs=True, **kw) for f, l in cases]
        replay_b = [model.attention_rescoring_batch(f, l, 4, lm=lm_b, use_graphs=True, **kw) for f, l in cases]
        plain = [model.attention_rescoring_batch(f, l, 4, use_graphs=True, ctc_weight=0.5, reverse_weight=0.3) for f, l in cases]
        monkeypatch.setattr(asr_model, "DEVICE_BEAM", False)
        host_a = [model.attention_rescoring_batch(f, l, 4, lm=lm_a, **kw) for f, l in cases]
    assert first_a == want_a and replay_a == want_a
    assert first_b == want_b and replay_b == want_b
    assert host_a == want_a
    assert want_a != want_b and want_a != plain                        # the two models really pick differently
    recs = model._decode_graphs
    assert sum(1 for k, v in recs.items() if k[0] == "s2" and v is not None and (k[6] is lm_a or k[6] is lm_b)) >= 2
    alive = weakref.ref(lm_a)                                          # the key holds the LM itself: the tables a cached capture
    del lm_a, recs                                                     # points at outlive the caller's reference
    gc.collect()
    assert any(k[0] == "s2" and k[6] is alive() is not None for k in model._decode_graphs)
