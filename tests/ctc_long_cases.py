"""Inputs and the float64 yardstick of the long-utterance CTC loss tests (test_ctc_long_ref.py on the CPU, test_ctc_long_gpu.py
on the device).  The yardstick is torch's own CTC loss in float64 on the CPU over log_softmax of the logits
(ctc_nbest_ref.nbest_grad with group = 1); it is handed the float32 logits the kernel reads, cast to float64.  Nothing here
touches the code under test."""
import torch

import ctc_nbest_ref as ref


class Case:
    """logits (B, T, V) float32, hlens / ylens (B) int32, ys (B, Lmax) int32 (valid token ids behind every length)."""

    def __init__(self, logits, hlens, ys, ylens):
        self.logits = logits.float().contiguous()
        self.hlens = torch.as_tensor(hlens, dtype=torch.int32)
        self.ys = ys.to(torch.int32).contiguous()
        self.ylens = torch.as_tensor(ylens, dtype=torch.int32)
        self.B, self.T, self.V = self.logits.shape
        self.Lmax = self.ys.shape[1]
        self._ref = None

    def yardstick(self):
        """-> nll (B) float64, 0 at an infeasible utterance;  d sum_b nll_b / d logits (B, T, V) float64, 0 at padded frames and
        infeasible utterances.  Computed once."""
        if self._ref is None:
            logp, dx = ref.nbest_grad(self.logits.double(), self.hlens.tolist(), self.ys, self.ylens, 1, -torch.ones(self.B, 1))
            logp = logp.view(-1)
            self._ref = (torch.where(torch.isfinite(logp), -logp, torch.zeros_like(logp)), dx)
        return self._ref

    def infeasible(self):
        return ref.infeasible_rows(self.hlens.tolist(), self.ys, self.ylens, 1, self.V, self.Lmax, self.T)


def targets(gen, B, Lmax, V, ylens, repeat_at=()):
    """Random targets without adjacent equal tokens, then an adjacent repeat forced at position repeat_at[b] of utterance b."""
    ys = torch.randint(1, V, (B, Lmax), generator=gen)
    for b in range(B):
        for i in range(1, Lmax):
            while ys[b, i] == ys[b, i - 1]:
                ys[b, i] = torch.randint(1, V, (1,), generator=gen)
    for b, k in enumerate(repeat_at):
        assert k + 1 < int(ylens[b])
        ys[b, k + 1] = ys[b, k]
        while k + 2 < Lmax and (ys[b, k + 2] == ys[b, k + 1] or (k + 3 < Lmax and ys[b, k + 2] == ys[b, k + 3])):
            ys[b, k + 2] = ys[b, k + 2] % (V - 1) + 1
    return ys


def random_case(B, T, V, Lmax, hlens, ylens, std, seed, repeat_at=()):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, V, generator=gen) * std
    return Case(logits, hlens, targets(gen, B, Lmax, V, ylens, repeat_at), ylens)


def flat(seed=0, std=6.0):
    """(B, T, V, Lmax) = (2, 1500, 64, 200), randn * 6: a long high-loss utterance and a short one in the same launch, one
    adjacent repeat in each target."""
    return random_case(2, 1500, 64, 200, [1500, 40], [200, 7], std, seed, repeat_at=(57, 3))


def peaked(seed=0):
    """The flat case with +14 along a valid alignment: in each of an utterance's L equal segments the label is held for about
    T / (2 L) frames, the rest of the segment is blank (so a repeated label has its blank).  The noise under the peak is
    randn * 2: nll is about 4 nats (under randn * 6 a +14 peak does not dominate its row, and the loss stays in the thousands)."""
    c = flat(seed, std=2.0)
    logits = c.logits.clone()
    for b in range(c.B):
        Tb, L = int(c.hlens[b]), int(c.ylens[b])
        hold = max(1, Tb // (2 * L))
        for t in range(Tb):
            seg = t * L // Tb
            first = -(-seg * Tb // L)                    # first frame of the segment
            logits[b, t, int(c.ys[b, seg]) if t - first < hold else 0] += 14.0
    return Case(logits, c.hlens, c.ys, c.ylens)


def single_alignment(seed=0):
    """V = 64, L = 255, three runs of equal tokens - a pair, a triple and a run of four: six adjacent repeats, each of which
    needs its blank - so L + 6 = 261 frames admit exactly ONE alignment (every label one frame, a blank only inside the runs).
    Utterance 0 has those 261 frames (gradient = softmax - onehot(path)), utterance 1 has 262 (many alignments), utterance 2
    has 260: infeasible.  -> (case, path (261) of utterance 0)."""
    V, L, T = 64, 255, 262
    gen = torch.Generator().manual_seed(seed)
    ys = targets(gen, 1, L, V, [L])
    for start, run in ((20, 2), (100, 3), (200, 4)):
        ys[0, start:start + run] = ys[0, start]
        for i in (start - 1, start + run):               # the run's neighbours differ from it and from their own neighbours
            while ys[0, i] == ys[0, i - 1] or ys[0, i] == ys[0, i + 1]:
                ys[0, i] = ys[0, i] % (V - 1) + 1
    tok = ys[0].tolist()
    repeats = sum(1 for i in range(1, L) if tok[i] == tok[i - 1])
    assert repeats == 6 and L + repeats == 261
    path = []
    for i, c in enumerate(tok):
        if i > 0 and tok[i - 1] == c:
            path.append(0)
        path.append(c)
    assert len(path) == 261
    logits = torch.randn(3, T, V, generator=gen) * 6.0
    return Case(logits, [261, 262, 260], ys.repeat(3, 1), [L, L, L]), torch.tensor(path)


def row_shift(seed=0):
    """(3, 70, 37, 5): utterance 0 with +3e4 on every logit, utterance 1 with -3e4 (a constant per row changes neither loss nor
    gradient; the yardstick reads the shifted float32 values)."""
    c = random_case(3, 70, 37, 5, [70, 51, 33], [5, 4, 5], 2.0, seed, repeat_at=(1,))
    logits = c.logits.clone()
    logits[0] += 3.0e4
    logits[1] -= 3.0e4
    return Case(logits, c.hlens, c.ys, c.ylens)


LADDER_T = (248, 400, 600, 800, 1000, 1500, 2000)


def ladder_point(T, seed):
    """B = 1, V = 3246 (the bench vocabulary), randn * 2, L = min(255, T // 6)."""
    L = min(255, T // 6)
    return random_case(1, T, 3246, L, [T], [L], 2.0, seed)
