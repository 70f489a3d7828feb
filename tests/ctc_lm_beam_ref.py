"""The yardstick for the LM-fused CTC prefix beam search: the reference's per-frame dict loop (asr_model.py:359-396) written
down as directly as possible in Python floats, with ONE change - the key that orders next_hyps before the cut to `beam`:

    total(p) = log_add(pb, pnb) + lm_weight * LM(p) + length_bonus * len(p)
    LM(p)    = sum over i < len(p), left to right, of log10 p(word(p_i) | h_i)        (ngram_ref.RefLM.p for every term)

Independent of openeat_amd: dicts keyed by token tuples, insertion order and Python's stable sort for ties, RefLM (a dict of
word tuples and the back-off recursion) for the LM.  LM(p) is memoised per prefix.  At the end of the utterance every
survivor gets the </s> term when eos, and the survivors are stably re-sorted by total.

Also here: the generator of the random test cases, shared by the CPU and the GPU tests."""
import math

import numpy as np

NEG = -math.inf


def log_add(xs):
    m = max(xs)
    if m == NEG:
        return NEG
    return m + math.log(sum(math.exp(x - m) for x in xs))


class PrefixLM:
    """LM(p) and the </s> term for token prefixes, through ngram_ref.RefLM; token2char: id -> string (a list)."""

    def __init__(self, ref, token2char):
        self.ref, self.t2c = ref, token2char
        self.memo = {(): 0.0}

    def word(self, tok):
        s = self.t2c[tok] if 0 <= tok < len(self.t2c) else None
        return s if (s,) in self.ref.grams else "<unk>"

    def context(self, prefix):
        seq = ["<s>"] + [self.word(t) for t in prefix]
        return tuple(seq[max(0, len(seq) - (self.ref.order - 1)):]) if self.ref.order > 1 else ()

    def lm(self, prefix):
        v = self.memo.get(prefix)
        if v is None:
            v = self.lm(prefix[:-1]) + self.ref.p(self.word(prefix[-1]), self.context(prefix[:-1]))[0]
            self.memo[prefix] = v
        return v

    def eos(self, prefix):
        return self.ref.p("</s>", self.context(prefix))[0]


def _gap(totals, beam, best):
    """Smallest non-zero relative gap between neighbours among the first beam+1 totals (sorted descending)."""
    head = [t for t in totals[:beam + 1] if t != NEG]
    for a, b in zip(head, head[1:]):
        g = (a - b) / max(1.0, abs(a))
        if g > 0.0:
            best = min(best, g)
    return best


def search(top_logp, top_idx, beam, plm, lm_weight, length_bonus=0.0, eos=True):
    """top_logp (T, beam) / top_idx (T, beam): the frame's top-k log-probabilities (any float sequence) and token ids, in
    the order the frame lists them -> ([(prefix, total, ctc, lm)] sorted by total, smallest non-zero relative gap)."""
    def total(prefix, ctc, lm):
        return ctc + lm_weight * lm + length_bonus * len(prefix)

    cur = [((), (0.0, NEG))]
    gap = math.inf
    for t in range(len(top_idx)):
        nxt = {}
        for j in range(len(top_idx[t])):
            s, ps = int(top_idx[t][j]), float(top_logp[t][j])
            for prefix, (pb, pnb) in cur:
                last = prefix[-1] if prefix else None
                if s == 0:
                    a, b = nxt.get(prefix, (NEG, NEG))
                    nxt[prefix] = (log_add([a, pb + ps, pnb + ps]), b)
                elif s == last:
                    a, b = nxt.get(prefix, (NEG, NEG))
                    nxt[prefix] = (a, log_add([b, pnb + ps]))
                    ext = prefix + (s,)
                    a, b = nxt.get(ext, (NEG, NEG))
                    nxt[ext] = (a, log_add([b, pb + ps]))
                else:
                    ext = prefix + (s,)
                    a, b = nxt.get(ext, (NEG, NEG))
                    nxt[ext] = (a, log_add([b, pb + ps, pnb + ps]))
        ranked = sorted(nxt.items(), key=lambda kv: total(kv[0], log_add(list(kv[1])), plm.lm(kv[0])), reverse=True)
        gap = _gap([total(p, log_add(list(v)), plm.lm(p)) for p, v in ranked], beam, gap)
        cur = ranked[:beam]
    out = []
    for prefix, (pb, pnb) in cur:
        ctc = log_add([pb, pnb])
        lm = plm.lm(prefix)
        if eos:
            lm = lm + plm.eos(prefix)
        out.append((prefix, total(prefix, ctc, lm), ctc, lm))
    out.sort(key=lambda h: h[1], reverse=True)
    gap = _gap([h[1] for h in out], beam, gap)
    return out, gap


# ---------------------------------------------------------------------------------------------------------------------
# the random cases: those of test_device_prefix_beam_equals_the_host_recursion, each with an ARPA order
CASES = [(5, 60, 50, 10, 1.0, 3), (8, 40, 6, 4, 0.3, 2), (3, 120, 12, 10, 3.0, 5), (4, 33, 40, 1, 1.0, 3), (2, 50, 300, 16, 2.0, 4),
         (6, 25, 5, 5, 0.0, 1)]
WEIGHTS = [(0.0, 0.0), (0.5, 0.0), (0.3, 0.8)]


def make_case(tmp_path, B, T, V, beam, sharp, order):
    """-> (logits (B, T, V) float32 torch tensor, lens (B) int32 tensor, ARPA path, token2char list of V strings)."""
    import torch
    import ngram_ref
    seed = B * 100 + T + V
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    nw = max(V - 1, 2)
    path = str(tmp_path / f"case{seed}_{order}.arpa")
    words = ngram_ref.random_arpa(path, order, nw, 40 * nw, rng)
    t2c = ["<blank>"] + [words[i % len(words)] for i in range(V - 2)] + ["oov"]
    logits = torch.randn(B, T, V, generator=g) * sharp
    logits[:, :, 0] += 1.0
    lens = torch.randint(max(1, T // 2), T + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = T
    if (B, T, V) == CASES[0][:3]:
        lens[1] = 0
    return logits, lens, path, t2c


def tie_case(tmp_path):
    """Uniform frames (every token, blank included, equally likely) and an order-1 ARPA in which every word and </s> has
    log10 p = -1: exact ties under fusion - three prefixes share the best total of the 25-frame utterance."""
    import torch
    import ngram_ref
    B, T, V, beam = 2, 25, 5, 5
    words = [f"w{i}" for i in range(V - 1)]
    path = str(tmp_path / "ties.arpa")
    ngram_ref.write_arpa(path, [[(("<s>",), -99.0, None), (("</s>",), -1.0, None), (("<unk>",), -1.0, None)]
                                + [((w,), -1.0, None) for w in words]])
    t2c = ["<blank>"] + words
    logits = torch.zeros(B, T, V)
    lens = torch.tensor([T, T - 7], dtype=torch.int32)
    return logits, lens, path, t2c, beam
