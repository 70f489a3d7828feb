"""The yardstick for the resumable CTC prefix beam search (oe_ctc_prefix_beam_chunk): the dict loop of
ctc_bias_beam_ref.search, restated so that it can stop after any frame and go on later, and so that it tracks, next to every
prefix, the emission frame of each of its tokens.  Nothing of openeat_amd; tests/test_ctc_stream_beam_ref.py pins it to
ctc_bias_beam_ref.search / ctc_lm_beam_ref.search.

Emission frames.  A prefix of next_hyps that is a current prefix (it stays, or an extension lands on it) keeps the frames it
has; any other is new, made by its one parent at frame t (the global frame index), and has the parent's frames followed by t.
So a prefix that left the beam and is made again gets the later frame.

Stable prefix.  After a chunk, the longest common prefix of the live prefixes' tokens; it only grows.  Where the live prefixes
disagree about the frame of a shared token, the earliest is committed.  The n-best reports the committed frames for the stable
tokens and the prefix' own for the rest."""
import math

import ctc_bias_beam_ref as BR
from ctc_lm_beam_ref import NEG, _gap, log_add


class Stream:
    """graph: a ctc_bias_beam_ref graph or None (no bias); plm: a ctc_lm_beam_ref.PrefixLM or None."""

    def __init__(self, beam, graph=None, plm=None, lm_weight=0.0, length_bonus=0.0, eos=True, final=True):
        self.beam, self.graph, self.plm = beam, graph, plm
        self.lm_weight, self.length_bonus, self.eos, self.final = lm_weight, length_bonus, eos, final
        self.cur = [((), (0.0, NEG))]
        self.frames = {(): ()}                                     # of the live prefixes
        self.t = 0
        self.stable_tokens, self.stable_frames = [], []
        self.gap = math.inf

    def _lm(self, prefix):
        return 0.0 if self.plm is None else self.plm.lm(prefix)

    def _bias(self, prefix, final=False):
        return 0.0 if self.graph is None else BR.bias(self.graph, prefix, final)

    def _total(self, prefix, ctc, lm, b):
        if self.plm is None:
            return (ctc + self.length_bonus * len(prefix)) + b
        return ((ctc + self.lm_weight * lm) + self.length_bonus * len(prefix)) + b

    def push(self, top_logp, top_idx):
        """The frames of one chunk (possibly none), then the commit of the stable prefix."""
        for f in range(len(top_idx)):
            nxt, made = {}, {}
            for j in range(len(top_idx[f])):
                s, ps = int(top_idx[f][j]), float(top_logp[f][j])
                for prefix, (pb, pnb) in self.cur:
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
                        made.setdefault(ext, prefix)
                    else:
                        ext = prefix + (s,)
                        a, b = nxt.get(ext, (NEG, NEG))
                        nxt[ext] = (a, log_add([b, pb + ps, pnb + ps]))
                        made.setdefault(ext, prefix)
            keyed = [(self._total(p, log_add(list(v)), self._lm(p), self._bias(p)), p, v) for p, v in nxt.items()]
            keyed.sort(key=lambda e: e[0], reverse=True)
            self.gap = _gap([e[0] for e in keyed], self.beam, self.gap)
            keyed = keyed[:self.beam]
            frames = {}
            for _, p, _ in keyed:
                frames[p] = self.frames[p] if p in self.frames else self.frames[made[p]] + (self.t,)
            self.cur = [(p, v) for _, p, v in keyed]
            self.frames = frames
            self.t += 1
        self._commit()

    def _commit(self):
        live = [p for p, _ in self.cur]
        n = min(len(p) for p in live)
        S = len(self.stable_tokens)
        while S < n and all(p[S] == live[0][S] for p in live):
            self.stable_tokens.append(live[0][S])
            self.stable_frames.append(min(self.frames[p][S] for p in live))
            S += 1

    def lcp(self):
        """The longest common prefix of the live prefixes, from their tokens alone."""
        live = [p for p, _ in self.cur]
        n = 0
        while all(len(p) > n for p in live) and all(p[n] == live[0][n] for p in live):
            n += 1
        return list(live[0][:n])

    def stable(self):
        return list(self.stable_tokens), list(self.stable_frames)

    def nbest(self, last):
        """-> ([(prefix, total, ctc, lm, bias)], [frames of each]).  last: the end-of-utterance steps (the </s> term, the pending
        credit dropped if final, the stable re-sort); otherwise the running totals in the search's own order."""
        out = []
        for prefix, (pb, pnb) in self.cur:
            ctc = log_add([pb, pnb])
            lm = self._lm(prefix)
            if last and self.eos and self.plm is not None:
                lm = lm + self.plm.eos(prefix)
            b = self._bias(prefix, last and self.final)
            out.append((prefix, self._total(prefix, ctc, lm, b), ctc, lm, b))
        if last:
            out.sort(key=lambda h: h[1], reverse=True)
            self.gap = _gap([h[1] for h in out], self.beam, self.gap)
        S = len(self.stable_tokens)
        return out, [self.stable_frames + list(self.frames[h[0]][S:]) for h in out]


def cut_sets(T):
    """The ways an utterance of T frames is cut in the tests: one chunk; every frame its own chunk; chunks of 1, 0, 5 frames and
    the rest (as far as T allows)."""
    a, b = min(1, T), min(6, T)
    return [[], list(range(1, T)), [a, a, b]]


LONG = (600, 12, 4, 6.0, 50)                                       # T, V, beam, sharpness, chunk: a prefix of some hundred tokens


def long_case():
    """-> logits (1, T, V): sharp posteriors without a favoured blank, so that nearly every frame emits a token."""
    import torch
    T, V, _, sharp, _ = LONG
    return torch.randn(1, T, V, generator=torch.Generator().manual_seed(T + V)) * sharp


def search(top_logp, top_idx, beam, cuts=None, **kw):
    """The whole utterance, cut into chunks at the frame indices `cuts` (None: one chunk) -> (n-best, frames, gap, per chunk
    the stable (tokens, frames))."""
    T = len(top_idx)
    edges = [0] + list(cuts or []) + [T]
    st = Stream(beam, **kw)
    stables = []
    for a, b in zip(edges, edges[1:]):
        st.push(top_logp[a:b], top_idx[a:b])
        stables.append(st.stable())
    nbest, frames = st.nbest(True)
    return nbest, frames, st.gap, stables
