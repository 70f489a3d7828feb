"""GPU: the front end's kernels (csrc/fbank.hip: fbank_kernel<128 / 256 / 512 / 1024>, its fused CMVN tail, utt_norm_kernel)
against the float64 yardstick of frontend_f64.py, on speech-like signals and at the kernels' loop and block boundaries.
* fbank: R <= 4 * R_ref with L = 4 (the error model and both constants: frontend_f64.py).  The oracle's R_ref is recomputed
  here and counts up to 0.6 only (it depends on the host's float32 FFT).  The margin of 4: a float32 emulation of the kernel's radix-2 Stockham FFT alone needs 1.34 x the oracle's R; the
  kernel's sequential mel accumulation and its wave-tree mean come on top.  At 4 x a loud bin is still held to about 1.5e-5.
* integer and layout properties: frame counts at the window's edges, zero padding frames, the floor, nothing written outside `out`.
* fused CMVN: bit for bit (plain - mean) * istd in float32 - a subtraction, then a product: nothing can contract.
* utt_norm_kernel: K <= 2 * K_ref at every length around its loops' steps (16 and 64 frames) and at widths with one, two and
  three column blocks, with lanes switched off; cells outside an utterance keep their bits.  T = 1 and zero-variance columns
  are 0/0 in the reference too and are out of scope."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frontend_f64 as Y  # noqa: E402
from openeat_amd.frontend import FLT_EPS, Fbank, utt_normalize_  # noqa: E402

DEV = "cuda"
TMAX = 1003                 # above the longest utterance, no multiple of the kernel's steps


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("config", Y.CONFIGS, ids=lambda c: "%dk-%dms-%d" % (c[0] // 1000, c[1], c[2]))
def test_fbank_vs_float64(config):
    rate, frame_ms, n_mel = config
    win, hop, nfft = Y.geometry(rate, frame_ms)
    ref = Y.fbank_reference(config, 0)
    names = list(ref)
    wav = torch.stack([ref[k][0] for k in names])
    fb = Fbank(n_mel, sample_rate=rate, frame_length_ms=frame_ms, device=DEV)
    assert (fb.win, fb.hop, fb.nfft) == (win, hop, nfft)
    feats, nfr = fb(wav.to(DEV))
    torch.cuda.synchronize()
    T = ref[names[0]][1].shape[0]
    assert feats.shape == (len(names), T, n_mel) and nfr.tolist() == [T] * len(names)
    feats = feats.cpu()
    bound = Y.fbank_bound()
    worst = {}
    for b, k in enumerate(names):
        _, m, mel64, E = ref[k]
        worst[k] = Y.fbank_excess(feats[b], m, mel64, E, nfft, 4.0)
    print("fbank %s (%d-point FFT): kernel R per signal %s; worst %.3f; R_ref %.3f, bound %.3f"
          % (config, nfft, {k: float("%.3g" % v) for k, v in worst.items()}, max(worst.values()), Y.r_ref(), bound))
    assert max(worst.values()) <= bound, worst


def _ragged(fb, lens, seed=5):
    g = torch.Generator().manual_seed(seed)
    wav = (torch.rand(len(lens), max(lens), generator=g) - 0.5) * 0.8       # live samples behind every length: they must not be read into a frame
    return wav, torch.tensor(lens, dtype=torch.int32)


def test_fbank_frame_counts_and_padding():
    """nsamples = win - 1, win, win + hop - 1, win + hop -> 0, 1, 1, 2 frames; frames at or past an utterance's end are exactly
    0; live frames are the oracle's."""
    rate, frame_ms, n_mel = Y.CONFIGS[0]
    fb = Fbank(n_mel, sample_rate=rate, frame_length_ms=frame_ms, device=DEV)
    lens = [fb.win - 1, fb.win, fb.win + fb.hop - 1, fb.win + fb.hop]
    wav, ns = _ragged(fb, lens)
    feats, nfr = fb(wav.to(DEV), ns.to(DEV))
    torch.cuda.synchronize()
    assert nfr.tolist() == [0, 1, 1, 2] and feats.shape == (4, 2, n_mel)
    none, nfr0 = fb(wav[:, : fb.win - 1].to(DEV))                           # a batch shorter than one window: no frame, no launch
    assert none.shape == (4, 0, n_mel) and nfr0.tolist() == [0, 0, 0, 0]
    feats = feats.cpu()
    for b, n in enumerate(nfr.tolist()):
        assert bool((_bits(feats[b, n:]) == 0).all()), b                    # +0.0, bit for bit
        if n:
            m, mel64, E = Y.fbank64(wav[b, : lens[b]], n_mel, rate, frame_ms)
            assert Y.fbank_excess(feats[b, :n], m, mel64, E, fb.nfft, 4.0) <= Y.fbank_bound()


def test_fbank_silence_is_the_floor():
    """Digital silence gives log(FLT_EPS), the float32 nearest to it, in every live cell (test_fbank_vs_float64 holds the floor
    to 4 ulp only).  A float32 log whose compensated last sum the compiler had fused was 1 ulp off here."""
    rate, frame_ms, n_mel = Y.CONFIGS[0]
    want = torch.tensor(FLT_EPS, dtype=torch.float32).log()
    assert float(want) == float(np.float32(math.log(FLT_EPS)))
    fb = Fbank(n_mel, sample_rate=rate, frame_length_ms=frame_ms, device=DEV)
    wav = torch.zeros(2, int(rate))
    feats, nfr = fb(wav.to(DEV), torch.tensor([int(rate), fb.win + 3 * fb.hop], device=DEV))
    torch.cuda.synchronize()
    assert nfr.tolist() == [98, 4]
    feats = feats.cpu()
    assert bool((feats[0] == want).all()) and bool((feats[1, :4] == want).all()) and bool((_bits(feats[1, 4:]) == 0).all())


@pytest.mark.parametrize("frames", [(7, 6, 5), (7, 5), (7,)], ids=lambda f: "B%d" % len(f))
def test_fbank_writes_nothing_outside_out(frames):
    """B * Tmax = 21, 14, 7: the last block of four waves has three, two and one waves without a frame.  `out` is a view of a
    larger NaN-filled buffer; every cell before and after the view stays NaN, every cell of it is written."""
    rate, frame_ms, n_mel = Y.CONFIGS[0]
    fb = Fbank(n_mel, sample_rate=rate, frame_length_ms=frame_ms, device=DEV)
    lens = [fb.win + (f - 1) * fb.hop + 7 for f in frames]
    wav, ns = _ragged(fb, lens)
    B, Tmax = len(frames), fb.num_frames(max(lens))
    assert Tmax == 7 and (B * Tmax) % 4 == {3: 1, 2: 2, 1: 3}[B]
    guard, cells = 4 * 64 * n_mel, B * Tmax * n_mel
    buf = torch.full((guard + cells + guard,), float("nan"), device=DEV)
    out = buf[guard: guard + cells].view(B, Tmax, n_mel)
    feats, nfr = fb(wav.to(DEV), ns.to(DEV), out=out)
    torch.cuda.synchronize()
    assert feats.data_ptr() == out.data_ptr() and nfr.tolist() == list(frames)
    buf = buf.cpu()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + cells:]).all())
    got = buf[guard: guard + cells].view(B, Tmax, n_mel)
    assert bool(torch.isfinite(got).all())
    plain, _ = fb(wav.to(DEV), ns.to(DEV))
    assert torch.equal(_bits(plain.cpu()), _bits(got))
    for b, n in enumerate(frames):
        assert bool((_bits(got[b, n:]) == 0).all())


def test_fused_cmvn_is_subtract_then_multiply():
    """For every utterance the fused output is (plain - mean) * istd in float32, bit for bit; padded frames stay exactly 0,
    not (0 - mean) * istd."""
    rate, frame_ms, n_mel = Y.CONFIGS[0]
    fb = Fbank(n_mel, sample_rate=rate, frame_length_ms=frame_ms, device=DEV)
    ref = Y.fbank_reference(Y.CONFIGS[0], 0)
    names = ["white 0.9", "tone+weak", "voiced gated", "dc+noise", "zeros"]
    wav = torch.stack([ref[k][0] for k in names])
    lens = [16000, 12345, 16000, 4000, 399]
    ns = torch.tensor(lens, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(11)
    mean = (15.0 * torch.randn(n_mel, generator=g)).to(DEV)
    istd = (torch.rand(n_mel, generator=g) * 3.0 + 0.05).to(DEV)
    plain, nfr = fb(wav.to(DEV), ns)
    fused, nfr2 = fb(wav.to(DEV), ns, cmvn=(mean, istd))
    torch.cuda.synchronize()
    assert nfr.tolist() == nfr2.tolist() == [98, 75, 98, 23, 0]
    want = (plain - mean) * istd
    for b, n in enumerate(nfr.tolist()):
        assert torch.equal(_bits(fused[b, :n]), _bits(want[b, :n])), names[b]
        assert bool((_bits(fused[b, n:]) == 0).all()), names[b]
    assert bool((fused[0, :98] != plain[0, :98]).any())


def _utt_batch(F, family):
    """The fourteen lengths as one ragged batch plus an utterance of no frames; cells outside an utterance hold a canary."""
    data = Y.utt_norm_data(F, family)
    lens = [x.shape[0] for x in data] + [0]
    g = torch.Generator().manual_seed(F)
    x = torch.randn(len(lens), TMAX, F, generator=g) * 100.0 + 12345.0
    for b, a in enumerate(data):
        x[b, : a.shape[0]] = torch.from_numpy(a.copy())
    return data, lens, x


@pytest.mark.parametrize("F", Y.UTT_WIDTHS)
def test_utt_norm_vs_float64(F):
    bound = Y.utt_norm_bound()
    worst = {}
    for family in Y.UTT_FAMILIES:
        data, lens, x = _utt_batch(F, family)
        got = utt_normalize_(x.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        got = got.cpu()
        for b, a in enumerate(data):
            T = a.shape[0]
            worst[family, T] = Y.utt_norm_excess(got[b, :T].numpy(), a)
        for b, T in enumerate(lens):                                        # an utterance's padding, and all of the empty one
            assert torch.equal(_bits(got[b, T:]), _bits(x[b, T:])), (family, T)
    per_family = {f: max(v for (ff, _), v in worst.items() if ff == f) for f in Y.UTT_FAMILIES}
    per_len = {T: max(v for (_, tt), v in worst.items() if tt == T) for T in Y.UTT_LENGTHS}
    print("utt_norm F=%d: kernel K per family %s, per length %s; worst %.3f; K_ref %.3f, bound %.3f"
          % (F, {k: float("%.3g" % v) for k, v in per_family.items()}, {k: float("%.3g" % v) for k, v in per_len.items()},
             max(worst.values()), Y.k_ref(), bound))
    assert max(worst.values()) <= bound, {k: v for k, v in worst.items() if v > bound}


@pytest.mark.parametrize("F", [65, 23])
def test_utt_norm_lengths_argument(F):
    """nframes = None normalises all Tmax frames; nframes[b] > Tmax behaves as Tmax."""
    bound = Y.utt_norm_bound()
    data = Y.utt_norm_data(F, "logmel")
    x = torch.stack([torch.from_numpy(data[Y.UTT_LENGTHS.index(129)].copy()), torch.from_numpy(data[Y.UTT_LENGTHS.index(1000)][:129].copy())])
    none = utt_normalize_(x.to(DEV))
    over = utt_normalize_(x.to(DEV), torch.tensor([130, 1 << 30], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(_bits(none.cpu()), _bits(over.cpu()))
    for b in range(2):
        assert Y.utt_norm_excess(none[b].cpu().numpy(), x[b].numpy()) <= bound
