"""CPU: pins the front end's float64 yardstick (frontend_f64.py) and proves that its error models have teeth.
* the float32 oracle stays inside the models on every signal (R_ref <= 0.6, K_ref <= 1.0): a condition on the inputs - if it
  fails, the signal set or the yardstick has drifted;
* float32 mutants of the oracle, one deliberate fault each, exceed the bounds the GPU tests use (4 * R_ref with L = 4;
  2 * K_ref: Y.fbank_bound(), Y.utt_norm_bound()), two of them while still passing the log-domain check of test_gpu_engine.py (rtol 2e-4, atol 2e-3)."""
import numpy as np
import pytest
import torch

import frontend_f64 as Y
from oracle import fbank as FB

WHITE = ("white 0.9", "white 0.01")


def _oracle(w, config):
    rate, frame_ms, n_mel = config
    return FB.fbank(w, num_mel_bins=n_mel, sample_rate=rate, frame_length_ms=frame_ms)


def _mutant_ratio(config, name, fault, seed=0):
    """(excess of the mutant / the GPU test's bound, the mutant's output, the oracle's) on one signal."""
    rate, frame_ms, n_mel = config
    w, m, mel64, E = Y.fbank_reference(config, seed)[name]
    got = Y.fbank32(w, n_mel, rate, frame_ms, fault=fault)
    return Y.fbank_excess(got, m, mel64, E, Y.geometry(rate, frame_ms)[2], 4.0) / Y.fbank_bound(), got, _oracle(w, config)


@pytest.mark.parametrize("config", Y.CONFIGS)
def test_fbank64_is_the_oracle_on_white_noise(config):
    """Where the log-domain check applies, the yardstick is the oracle within that check; the float32 restatement the mutants
    are cut from is the oracle bit for bit."""
    for seed in Y.SEEDS:
        for name in WHITE:
            w, m, _, _ = Y.fbank_reference(config, seed)[name]
            ref = _oracle(w, config)
            np.testing.assert_allclose(m.log().numpy(), ref.numpy(), rtol=2e-4, atol=2e-3)
            assert torch.equal(Y.fbank32(w, config[2], config[0], config[1]), ref)


def test_signals_and_geometry():
    assert [Y.geometry(c[0], c[1])[2] for c in Y.CONFIGS] == [512, 256, 512, 512, 1024, 128]
    for rate in (8000.0, 16000.0):
        s = Y.signals(rate, 0)
        assert len(s) == 12
        for name, w in s.items():
            assert w.dtype == torch.float32 and w.shape == (int(rate),) and float(w.min()) >= -1.0 and float(w.max()) < 1.0, name
    # half of the gated signal's frames and all of the silent one's sit on the floor; E is the raw energy, DC included
    _, m, mel64, E = Y.fbank_reference(Y.CONFIGS[0], 0)["voiced gated"]
    floored = (mel64 <= Y.FLT_EPS).all(dim=1).double().mean()
    assert 0.3 < float(floored) < 0.6
    assert bool((m >= Y.FLT_EPS).all())
    _, m, mel64, E = Y.fbank_reference(Y.CONFIGS[0], 0)["zeros"]
    assert bool((m == Y.FLT_EPS).all()) and bool((E == 0).all())
    _, _, _, E = Y.fbank_reference(Y.CONFIGS[0], 0)["dc+noise"]
    np.testing.assert_allclose(E.numpy(), 400 * (0.5 * 32768.0) ** 2, rtol=1e-3)


def test_r_ref():
    """The float32 oracle needs R <= 0.6 (L = 1) on every signal, both seeds, all six configurations.
    Host-dependent through torch's float32 FFT and matrix product: 0.517 on the host the tables of frontend_f64.py are from
    (the chirp at 16k/25/80); 0.933 on an EPYC 9575F (the chirp at 8k/10/23, a 128-point FFT; 0.610 at 16k/20/80), where this
    test fails.  The bound is the one the yardstick was specified with and stays: a kernel's allowance is cut from it."""
    table = Y.r_ref_table()
    assert len(table) == 6 * 12
    for key, r in sorted(table.items(), key=lambda kv: -kv[1])[:5]:
        print(key, "R = %.3f" % r)
    print("R_ref = %.3f" % Y.r_ref())
    assert Y.r_ref() <= Y.R_REF_MAX == 0.6
    assert Y.r_ref() >= 0.05          # a yardstick ten times looser than the oracle's own round-off has drifted as well


def test_k_ref():
    """numpy's float32 normalisation needs K <= 1.0 on every length, width and data family."""
    table = Y.k_ref_table()
    assert len(table) == 4 * 5
    for key, k in sorted(table.items()):
        print(key, "K = %.3f" % k)
    print("K_ref = %.3f" % Y.k_ref())
    assert Y.k_ref() <= Y.K_REF_MAX == 1.0
    assert Y.k_ref() >= 0.1
    x = Y.utt_norm_data(65, "mixed")[5]
    assert np.array_equal(Y.utt_norm32(x), FB.utt_normalize(torch.from_numpy(x.copy())).numpy())
    np.testing.assert_allclose(Y.utt_norm64(x).mean(axis=0), 0.0, atol=1e-12)
    np.testing.assert_allclose(Y.utt_norm64(x).std(axis=0), 1.0, rtol=1e-12)


@pytest.mark.parametrize("fault", [f for f in Y.FBANK_MUTANTS if f != "preemph0"])
def test_fbank_mutant_exceeds_the_gpu_bound(fault):
    """Under every configuration the mutant misses 4 * R_ref (L = 4) on at least one signal of the set."""
    for config in Y.CONFIGS:
        ratios = {name: _mutant_ratio(config, name, fault)[0] for name in Y.signals(config[0], 0)}
        print(fault, config, {k: float("%.3g" % v) for k, v in ratios.items()})
        assert max(ratios.values()) > 1.0, (fault, config)


def test_fbank_mutant_preemph0_is_hidden_by_the_window():
    """The fifth mutant cannot be seen by any test of the output: the symmetric Hann window's first tap is exactly 0, so
    whatever the first sample's pre-emphasis predecessor is, the product is 0.  Asserted so that a window with a live first
    tap (a periodic one, say) does not get in unnoticed: then this mutant belongs with the four above."""
    for config in Y.CONFIGS:
        rate, frame_ms, n_mel = config
        assert float(FB.povey_window(Y.geometry(rate, frame_ms)[0])[0]) == 0.0
        for name, (w, _, _, _) in Y.fbank_reference(config, 0).items():
            assert torch.equal(Y.fbank32(w, n_mel, rate, frame_ms, fault="preemph0"), _oracle(w, config)), (config, name)


@pytest.mark.parametrize("config", Y.CONFIGS)
def test_gain_mutant_passes_the_log_check_and_misses_the_new_one(config):
    """A gain error of 1e-4: invisible to rtol 2e-4 / atol 2e-3 on the log-mel output (on every signal), far outside the
    power-domain bound on white noise."""
    for name in Y.signals(config[0], 0):
        ratio, got, ref = _mutant_ratio(config, name, "gain")
        assert Y.passes_log_check(got, ref), name
        if name in WHITE:
            print(config, name, "gain mutant: %.1f x the bound" % ratio)
            assert ratio > 10.0, (name, ratio)


@pytest.mark.parametrize("config", Y.CONFIGS)
def test_leak_mutant_passes_the_log_check_on_white_noise_and_misses_the_new_one_on_a_tone(config):
    """1e-9 of the frame's energy in every FFT bin: white noise has no bin quiet enough to show it to the log-domain check; a
    tone's quiet bins show it to the power-domain bound (and would to the log-domain one, which cannot be used there: the
    float32 oracle itself misses it on a tone)."""
    ratio, got, ref = _mutant_ratio(config, "white 0.9", "leak")
    assert Y.passes_log_check(got, ref)
    ratio, got, ref = _mutant_ratio(config, "tone", "leak")
    print(config, "leak mutant on the tone: %.1f x the bound" % ratio)
    assert ratio > 2.0, ratio


def test_log_check_cannot_judge_the_oracle_on_speech_like_signals():
    """Why the log-domain check stays on white noise: against float64 the float32 oracle itself misses it on a tone, a tone
    with a faint second one, a chirp and DC plus faint noise - while it sits inside the power-domain model (test_r_ref)."""
    config = Y.CONFIGS[0]
    for name in ("tone", "tone+weak", "chirp", "dc+noise"):
        w, m, _, _ = Y.fbank_reference(config, 0)[name]
        assert not Y.passes_log_check(_oracle(w, config), m.log()), name


@pytest.mark.parametrize("fault", Y.UTT_MUTANTS)
def test_utt_norm_mutant_exceeds_the_gpu_bound(fault):
    """Every normalisation mutant misses 2 * K_ref in every data family and at every width (at some length)."""
    bound = Y.utt_norm_bound()
    for F in Y.UTT_WIDTHS:
        for family in Y.UTT_FAMILIES:
            worst = max(Y.utt_norm_excess(Y.utt_norm32(x, fault, tmax=1003), x) for x in Y.utt_norm_data(F, family))
            assert worst > bound, (fault, F, family, worst)
