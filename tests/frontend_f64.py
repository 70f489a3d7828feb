"""Float64 yardstick for the acoustic front end (fbank, per-utterance normalisation), its error models, the signal set, and
float32 mutants that the error models must catch.  Imports the oracle only, never the package under test.
`python tests/frontend_f64.py` prints the tables below.

fbank.  A float32 front end cannot be judged in the log domain on speech-like signals: a quiet mel bin next to a loud one
carries the loud one's round-off, and the log amplifies it (the float32 oracle is 0.02 - 0.17 from float64 on a tone, a chirp,
DC plus a faint signal; a kernel has the same right).  The round-off of the mean, the window product and the FFT is an
error of about 2^-24 * sqrt(nfft * E) in every FFT bin's AMPLITUDE, E = the frame's raw energy sum((scale * x)^2), so
in a mel POWER m it is 2 * sqrt(m) * delta + delta^2.  fbank_excess() returns the smallest R with, for every element,

    |exp(got) - m| <= R * (2 * sqrt(mel64) * delta + delta^2) + L * 2^-23 * max(1, |ln m|) * m,   delta = 2^-24 * sqrt(nfft * E)

where m = max(mel64, FLT_EPS) and the second term is the rounding of the stored float32 log and of the log function itself
(L = 1 for a correctly rounded log; L = 4 for the kernel: v_log_f32 is good to 1 ulp of the log2, the scaling by ln 2 and the
float32 store add under 3 ulp of ln m - derived, not measured).

R of oracle/fbank.py (float32 torch, L = 1) against fbank64, worst of seeds 0 and 1, per signal and configuration
(rate, frame ms, mel bins); R_ref is the worst of all, and test_frontend_f64_ref.py asserts R_ref <= 0.6.  The figures depend
on the host's float32 FFT and matrix product.  These are from an x86 host on which torch reports AVX512 and MKL; an EPYC 9575F
with the same torch gave R_ref = 0.933 (the chirp at 8k/10/23, 0.610 at 16k/20/80, everything else under 0.51), and there the
assertion fails.  A kernel's bound, fbank_bound(), counts R_ref up to 0.6 only.  On MI355X fbank_kernel needed 0.61, 0.41,
0.52, 0.40, 0.19 and 0.49 under the six configurations (L = 4), the chirp every time.

    signal          16k/25/80  8k/25/40  16k/20/80  16k/32/64  16k/50/80  8k/10/23
    white 0.9          0.145     0.161     0.156     0.092     0.102     0.196
    white 0.01         0.146     0.184     0.170     0.178     0.112     0.185
    tone               0.058     0.119     0.069     0.046     0.033     0.120
    tone+weak          0.065     0.127     0.114     0.052     0.049     0.126
    voiced gated       0.040     0.041     0.126     0.083     0.031     0.067
    dc+noise           0.009     0.006     0.010     0.004     0.001     0.015
    dc-0.9+tone        0.005     0.006     0.004     0.006     0.003     0.005
    lsb                0.213     0.190     0.193     0.208     0.117     0.310
    square             0.033     0.041     0.038     0.103     0.016     0.000
    chirp              0.517     0.490     0.424     0.324     0.252     0.357
    impulse            0.117     0.044     0.165     0.111     0.111     0.028
    zeros              0.000     0.000     0.000     0.000     0.000     0.000
    R_ref = 0.517

Per-utterance normalisation.  z = (x - mean) / std (ddof 0) in float64; utt_norm_excess() returns the smallest K with

    |got - z| <= K * 2^-24 * ((|x| + sqrt(T) * rms_col) / sigma + (1 + sqrt(T)) * |z|)

(the mean's round-off is 2^-24 * sqrt(T) * rms_col for a float32 sum of T terms, the subtraction's 2^-24 * |x|, both divided
by sigma; the variance sum, the square root and the product are relative errors of z).  T = 1 and zero-variance columns are
0/0 in the reference as well and are not part of the set.

K of oracle/fbank.py::utt_normalize (numpy float32) over T in UTT_LENGTHS, worst per data family and F; K_ref is the worst
of all, and test_frontend_f64_ref.py asserts K_ref <= 1.0 (the same on both hosts; utt_norm_kernel on MI355X: 0.82 at worst):

    family         F=80   F=23   F=64   F=65  F=130
    logmel      0.676  0.672  0.608  0.696  0.789
    offset      0.716  0.618  0.729  0.629  0.685
    zero-mean   0.612  0.499  0.453  0.473  0.492
    mixed       0.782  0.635  0.767  0.845  0.748
    K_ref = 0.845
"""
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import fbank as FB  # noqa: E402

FLT_EPS = FB.FLT_EPS
# (sample rate, frame length ms, mel bins): FFTs of 512, 256, 512, 512, 1024 and 128 points
CONFIGS = [(16000.0, 25.0, 80), (8000.0, 25.0, 40), (16000.0, 20.0, 80), (16000.0, 32.0, 64), (16000.0, 50.0, 80), (8000.0, 10.0, 23)]
SEEDS = (0, 1)
UTT_LENGTHS = (2, 3, 15, 16, 17, 47, 48, 49, 63, 64, 65, 128, 129, 1000)
UTT_WIDTHS = (80, 23, 64, 65, 130)
UTT_FAMILIES = ("logmel", "offset", "zero-mean", "mixed")
FBANK_MUTANTS = ("window", "preemph0", "nomean", "gain", "leak")
UTT_MUTANTS = ("ddof1", "mean-short", "mean-tmax")
R_REF_MAX, K_REF_MAX = 0.6, 1.0         # what the float32 references may need (test_frontend_f64_ref.py)


def geometry(sample_rate, frame_length_ms, frame_shift_ms=10.0):
    """-> (window samples, hop samples, FFT points)."""
    win, hop = int(sample_rate * frame_length_ms * 0.001), int(sample_rate * frame_shift_ms * 0.001)
    return win, hop, max(128, FB._next_pow2(win))


# ---------------------------------------------------------------------------------------------------------------- fbank
def fbank64(wav, num_mel_bins=80, sample_rate=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemph=0.97, scale=32768.0):
    """oracle.fbank.fbank with every operation in float64, on the oracle's float32 tables upcast (the tables are part of the
    operation's definition).  wav (N,) -> (m (T, n_mel) = max(mel64, FLT_EPS), mel64 (T, n_mel), E (T, 1) = the frame's raw
    energy sum((scale * x)^2), before DC removal)."""
    x = wav.to(torch.float64) * scale
    win, hop, nfft = geometry(sample_rate, frame_length_ms, frame_shift_ms)
    T = FB.num_frames(x.numel(), win, hop)
    if T == 0:
        return torch.empty(0, num_mel_bins, dtype=torch.float64), torch.empty(0, num_mel_bins, dtype=torch.float64), torch.empty(0, 1, dtype=torch.float64)
    fr = x.as_strided((T, win), (hop, 1)).clone()
    E = (fr * fr).sum(dim=1, keepdim=True)
    fr = fr - fr.mean(dim=1, keepdim=True)
    prev = torch.cat([fr[:, :1], fr[:, :-1]], dim=1)
    fr = fr - preemph * prev
    fr = fr * FB.povey_window(win).to(torch.float64).unsqueeze(0)
    fr = torch.nn.functional.pad(fr, (0, nfft - win))
    spec = torch.fft.rfft(fr)
    power = spec.real * spec.real + spec.imag * spec.imag
    mel64 = power @ FB.mel_banks(num_mel_bins, nfft, sample_rate).to(torch.float64).T
    return torch.clamp(mel64, min=FLT_EPS), mel64, E


def fbank_excess(got_log, m, mel64, E, nfft, L):
    """The smallest R for which every element of got_log (T, n_mel; a log-mel output) meets the module docstring's bound.  In
    float64, over all elements; inf where the power-domain term is zero (digital silence) and the log term alone is missed."""
    got = torch.as_tensor(got_log).to(torch.float64)
    assert got.shape == m.shape, (got.shape, m.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    delta = 2.0 ** -24 * torch.sqrt(nfft * E)
    d = (got.exp() - m).abs()
    slack = L * 2.0 ** -23 * torch.clamp(m.log().abs(), min=1.0) * m
    a = (2.0 * torch.sqrt(mel64) * delta + delta * delta).expand_as(d)
    over = (d - slack).clamp_min(0.0)
    need = torch.where(over > 0, over / a, torch.zeros_like(over))      # over > 0, a == 0 -> inf
    return float(need.max())


def passes_log_check(got_log, ref_log, rtol=2e-4, atol=2e-3):
    """The log-domain check of test_gpu_engine.py (numpy.testing.assert_allclose's rule)."""
    got, ref = torch.as_tensor(got_log).to(torch.float64), torch.as_tensor(ref_log).to(torch.float64)
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def signals(sample_rate, seed):
    """name -> 1 s waveform in [-1, 1), float32."""
    sr = float(sample_rate)
    g = torch.Generator().manual_seed(seed)
    n = int(sr * 1.0)
    t = torch.arange(n) / sr
    s = {}
    s["white 0.9"] = (torch.rand(n, generator=g) - 0.5) * 0.9
    s["white 0.01"] = (torch.rand(n, generator=g) - 0.5) * 0.01
    s["tone"] = 0.5 * torch.sin(2 * math.pi * 440 * t)
    s["tone+weak"] = 0.5 * torch.sin(2 * math.pi * 440 * t) + 1e-3 * torch.sin(2 * math.pi * 0.19 * sr * t)
    f0 = 120
    harm = sum(torch.sin(2 * math.pi * f0 * h * t) / h ** 2 for h in range(1, int(sr / 2 / f0) - 1))      # 1/h^2 roll-off up to Nyquist
    gate = (torch.sin(2 * math.pi * 3 * t) > 0).float()                                                   # half the frames are digital silence
    s["voiced gated"] = 0.3 * harm / harm.abs().max() * gate
    s["dc+noise"] = 0.5 + (torch.rand(n, generator=g) - 0.5) * 1e-4
    s["dc-0.9+tone"] = -0.9 + 0.05 * torch.sin(2 * math.pi * 1000 * t)
    s["lsb"] = torch.randint(-1, 2, (n,), generator=g).float() / 32768
    s["square"] = torch.sign(torch.sin(2 * math.pi * 200 * t)) * 0.999
    s["chirp"] = 0.8 * torch.sin(2 * math.pi * (50 * t + 0.24 * sr * t * t))                              # 50 Hz -> 0.48 * rate
    imp = torch.zeros(n)
    imp[::997] = 0.9
    s["impulse"] = imp
    s["zeros"] = torch.zeros(n)
    return {k: v.to(torch.float32) for k, v in s.items()}


@functools.lru_cache(maxsize=None)
def fbank_reference(config, seed):
    """name -> (wav, m, mel64, E) of signals(rate, seed) under `config`; made once, nothing writes to it."""
    rate, frame_ms, n_mel = config
    return {k: (w,) + fbank64(w, n_mel, rate, frame_ms) for k, w in signals(rate, seed).items()}


@functools.lru_cache(maxsize=None)
def r_ref_table():
    """(config, signal) -> R of the float32 oracle (L = 1) against fbank64, worst of SEEDS."""
    table = {}
    for config in CONFIGS:
        rate, frame_ms, n_mel = config
        nfft = geometry(rate, frame_ms)[2]
        for seed in SEEDS:
            for name, (w, m, mel64, E) in fbank_reference(config, seed).items():
                got = FB.fbank(w, num_mel_bins=n_mel, sample_rate=rate, frame_length_ms=frame_ms)
                table[config, name] = max(table.get((config, name), 0.0), fbank_excess(got, m, mel64, E, nfft, 1.0))
    return table


def r_ref():
    return max(r_ref_table().values())


def fbank_bound():
    """The R a kernel may need (with L = 4): four times the oracle's.  The oracle's own R depends on the host's FFT and matrix
    product (0.52 and 0.93 were seen on two hosts, both on the chirp), so it counts up to R_REF_MAX only."""
    return 4.0 * min(r_ref(), R_REF_MAX)


def fbank32(wav, num_mel_bins=80, sample_rate=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemph=0.97, scale=32768.0,
            fault=None):
    """oracle.fbank.fbank restated in float32 (fault None: the same numbers), with one deliberate fault of FBANK_MUTANTS:
    window   - a periodic instead of a symmetric Hann window;
    preemph0 - the first sample's pre-emphasis predecessor is 0, not the sample itself;
    nomean   - no frame-mean removal;
    gain     - mel power times 1 + 1e-4;
    leak     - 1e-9 of the frame's spectral energy sum_k |X_k|^2 / nfft (by Parseval the energy of the windowed frame) added to
               every FFT bin's power.
    preemph0 changes no output: the symmetric Hann window's first tap is exactly 0, so the first sample's pre-emphasis never
    reaches the FFT.  It stays in the list so that test_frontend_f64_ref.py notices if the window ever stops hiding it."""
    assert fault is None or fault in FBANK_MUTANTS, fault
    x = wav.to(torch.float32) * scale
    win, hop, nfft = geometry(sample_rate, frame_length_ms, frame_shift_ms)
    T = FB.num_frames(x.numel(), win, hop)
    fr = x.as_strided((T, win), (hop, 1)).clone()
    if fault != "nomean":
        fr = fr - fr.mean(dim=1, keepdim=True)
    first = torch.zeros_like(fr[:, :1]) if fault == "preemph0" else fr[:, :1]
    prev = torch.cat([first, fr[:, :-1]], dim=1)
    fr = fr - preemph * prev
    window = torch.hann_window(win, periodic=True, dtype=torch.float32).pow(0.85) if fault == "window" else FB.povey_window(win)
    fr = fr * window.unsqueeze(0)
    fr = torch.nn.functional.pad(fr, (0, nfft - win))
    power = torch.fft.rfft(fr).abs().pow(2.0)
    if fault == "leak":
        power = power + 1e-9 * (2.0 * power.sum(dim=1, keepdim=True) - power[:, :1] - power[:, -1:]) / nfft
    mel = power @ FB.mel_banks(num_mel_bins, nfft, sample_rate).T
    if fault == "gain":
        mel = mel * (1.0 + 1e-4)
    return torch.max(mel, torch.tensor(FLT_EPS)).log()


# ------------------------------------------------------------------------------------------- per-utterance normalisation
def utt_norm64(x):
    """(x - mean) / std over the rows of x (T, F), ddof 0, in float64."""
    x64 = np.asarray(x, dtype=np.float64)
    return (x64 - x64.mean(axis=0)) / x64.std(axis=0)


def utt_norm_excess(got, x64):
    """The smallest K for which every element of got (T, F) meets the module docstring's bound; x64 is the input."""
    x64 = np.asarray(x64, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == x64.shape, (got.shape, x64.shape)
    if not np.isfinite(got).all():
        return math.inf
    T = x64.shape[0]
    sd = x64.std(axis=0)
    z = (x64 - x64.mean(axis=0)) / sd
    rms = np.sqrt((x64 * x64).mean(axis=0))
    g = math.sqrt(T)
    bound = 2.0 ** -24 * ((np.abs(x64) + g * rms) / sd + (1.0 + g) * np.abs(z))
    return float((np.abs(got - z) / bound).max())


@functools.lru_cache(maxsize=None)
def utt_norm_data(F, family):
    """A tuple of float32 arrays (T, F), one for each T of UTT_LENGTHS; no column of any has zero variance."""
    rng = np.random.default_rng(1000 * UTT_FAMILIES.index(family) + F)
    out = []
    for T in UTT_LENGTHS:
        for _ in range(100):        # at T = 2 the two float32 values of an "offset" column are now and then the same number: draw again
            r = rng.standard_normal((T, F))
            if family == "logmel":
                x = 15.0 + 3.0 * r
            elif family == "offset":
                x = 1000.0 + 0.01 * r
            elif family == "zero-mean":
                x = r
            else:                                               # per-column scales 2^+-6, means +-20
                x = r * np.exp2(rng.integers(-6, 7, (1, F))) + rng.standard_normal((1, F)) * 20.0
            x = x.astype(np.float32)
            if (x.astype(np.float64).std(axis=0) > 0).all():
                break
        assert (x.astype(np.float64).std(axis=0) > 0).all(), (family, T, F)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def k_ref_table():
    """(family, F) -> K of the numpy float32 oracle against utt_norm64, worst of UTT_LENGTHS."""
    table = {}
    for F in UTT_WIDTHS:
        for family in UTT_FAMILIES:
            table[family, F] = max(utt_norm_excess(FB.utt_normalize(torch.from_numpy(x.copy())).numpy(), x) for x in utt_norm_data(F, family))
    return table


def k_ref():
    return max(k_ref_table().values())


def utt_norm_bound():
    """The K a kernel may need: twice the oracle's, which counts up to K_REF_MAX only."""
    return 2.0 * min(k_ref(), K_REF_MAX)


def utt_norm32(x, fault=None, tmax=None):
    """oracle.fbank.utt_normalize restated in numpy float32 (fault None: the same numbers), with one fault of UTT_MUTANTS:
    ddof1      - the sample instead of the population standard deviation;
    mean-short - the mean taken without the last frame;
    mean-tmax  - the column sum divided by the padded length `tmax`, not by the utterance's own."""
    assert fault is None or fault in UTT_MUTANTS, fault
    a = np.asarray(x, dtype=np.float32)
    T = a.shape[0]
    if fault == "mean-short":
        mean = np.mean(a[:-1], axis=0)
    elif fault == "mean-tmax":
        mean = np.sum(a, axis=0) / np.float32(tmax)
    else:
        mean = np.mean(a, axis=0)
    if fault is None:
        return (a - mean) / np.std(a, axis=0)
    d = a - mean
    return d / np.sqrt(np.sum(d * d, axis=0) / np.float32(T - 1 if fault == "ddof1" else T))


def _print_tables():
    rt, kt = r_ref_table(), k_ref_table()
    names = list(signals(8000.0, 0))
    print("    signal          " + "  ".join("%dk/%d/%d" % (c[0] // 1000, c[1], c[2]) for c in CONFIGS))
    for n in names:
        print("    %-14s" % n + "".join("%10.3f" % rt[c, n] for c in CONFIGS))
    print("    R_ref = %.3f" % r_ref())
    print("    family      " + "".join("%7s" % ("F=%d" % F) for F in UTT_WIDTHS))
    for fam in UTT_FAMILIES:
        print("    %-10s" % fam + "".join("%7.3f" % kt[fam, F] for F in UTT_WIDTHS))
    print("    K_ref = %.3f" % k_ref())


if __name__ == "__main__":
    _print_tables()
