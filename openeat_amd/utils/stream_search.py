"""The resumable CTC prefix beam search as an object (oe_ctc_prefix_beam_chunk; semantics in include/openeat_hip.h): a
PrefixBeamStream owns what the search keeps between two chunks - the two states it ping-pongs between, the stable prefix and
its frames, the n-best buffers and a workspace sized by the largest chunk seen - and takes the frames chunk by chunk.  All
arithmetic is the kernel's; this is allocation and the copies to the host."""
from typing import Optional

import torch

from openeat_amd import hip


class PrefixBeamStream:
    """One batch of B recordings searched chunk by chunk with beam `beam`; max_len bounds the tokens of a prefix (one per
    frame at the most).  lm: an NgramLM, context: a ContextGraph, as the one-shot searches take them; without either the
    weights must be 0."""

    def __init__(self, B: int, beam: int, max_len: int, device, lm=None, context=None, lm_weight: float = 0.0,
                 length_bonus: float = 0.0, eos: bool = True, final: bool = True):
        self.spec = hip.PrefixSearch(beam, lm, context, lm_weight, length_bonus, eos, final)
        self.spec.validate("PrefixBeamStream", True)
        if B < 1 or max_len < 1:
            raise ValueError(f"PrefixBeamStream: bad shape B={B} max_len={max_len}")
        self.B, self.beam, self.max_len, self.device = B, beam, max_len, torch.device(device)
        dev = self.device
        self._abi = self.spec.abi(dev)
        n = hip.lib().oe_ctc_prefix_beam_state_bytes(B, beam, max_len)
        self._states = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.stable_prefix = torch.zeros(B, max_len, dtype=torch.int32, device=dev)
        self.stable_frame = torch.zeros(B, max_len, dtype=torch.int32, device=dev)
        self.stable_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.prefixes = torch.zeros(B, beam, max_len, dtype=torch.int32, device=dev)
        self.frames = torch.zeros(B, beam, max_len, dtype=torch.int32, device=dev)
        self.plen = torch.full((B, beam), -1, dtype=torch.int32, device=dev)
        self.total, self.ctc, self.lms, self.bias = (torch.zeros(B, beam, dtype=torch.float64, device=dev) for _ in range(4))
        # what the kernel is handed of the four, and what a result shows: an unwritten buffer stays zero, plain: ctc is the total
        self._outs, self.scores = self.spec.bind(dict(zip(hip.SCORES, (self.total, self.ctc, self.lms, self.bias))))
        self._ws, self._ws_T = None, -1
        self.reset()

    @classmethod
    def of(cls, spec, B: int, max_len: int, device):
        """The stream of `spec`, a hip.PrefixSearch built elsewhere."""
        return cls(B, spec.beam, max_len, device, spec.lm, spec.context, spec.lm_weight, spec.length_bonus, spec.eos, spec.final)

    def reset(self):
        """Back to the empty prefix: the next push starts a new search."""
        self._cur = None                                           # the state the next chunk resumes from (None: the start)
        self._flip = 0
        self.done = False
        self.stable_len.zero_()
        self._ws_T = -1                                            # the status word is zeroed again

    def _workspace(self, T: int):
        words = hip.lib().oe_ctc_prefix_beam_workspace_bytes(self.B, T, self.beam) // 4
        if self._ws is None or self._ws.numel() < words:
            self._ws = torch.empty(words, dtype=torch.int32, device=self.device)
            self._ws_T = -1
        if T != self._ws_T:                                        # the status word sits behind the chunk's back-pointers
            self._ws[words - 1: words].zero_()
            self._ws_T = T
        return self._ws, self._ws[words - 1: words]

    def push(self, top_logp: torch.Tensor, top_idx: torch.Tensor, lens: Optional[torch.Tensor] = None, last: bool = False,
             emit: bool = True, raw: bool = False):
        """The next chunk: top_logp (B, T, beam) float32 / top_idx (B, T, beam) int64 as ops.topk_rows gives them, lens (B) int32
        the chunk's frames per recording (None: T; 0: the recording rests).  last: the audio ends here.  emit: also write the
        n-best.  -> per recording {"nbest": [(prefix, total, ctc, lm, bias)] (empty without emit / last), "frames": the
        emission frames of each of its prefixes, "stable": (tokens, frames)}; one copy to the host, which drains the stream.
        raw=True: no copy and no wait - a dict of the device tensors (prefixes, frames, plen, total, ctc, lm, bias, stable_prefix,
        stable_frame, stable_len, status), which the next push overwrites; the caller checks `status` after its own wait."""
        if self.done:
            raise RuntimeError("PrefixBeamStream.push: the search has ended (last was given); reset() starts the next")
        if not (top_logp.is_cuda and top_idx.is_cuda and top_logp.dtype == torch.float32 and top_idx.dtype == torch.int64):
            raise TypeError("PrefixBeamStream.push: float32 / int64 CUDA tensors required")
        if top_logp.dim() != 3 or top_logp.shape[0] != self.B or top_logp.shape[2] != self.beam or top_idx.shape != top_logp.shape:
            raise ValueError(f"PrefixBeamStream.push: top-k of shape ({self.B}, T, {self.beam}) required (got {tuple(top_logp.shape)})")
        top_logp, top_idx = top_logp.contiguous(), top_idx.contiguous()
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        ws, status = self._workspace(top_logp.shape[1])
        a = hip.prefix_beam_args(top_logp, top_idx, lens, self.beam, self.max_len, ws, self.prefixes, self.plen, *self._outs,
                                 **self._abi)
        out = self._states[self._flip]
        hip.prefix_beam_chunk(a, self._cur, out, self.stable_prefix, self.stable_frame, self.stable_len, self.frames, last=last, emit=emit)
        self._cur, self._flip = out, self._flip ^ 1
        self.done = bool(last)
        wrote = emit or last
        tensors = dict(prefixes=self.prefixes, frames=self.frames, plen=self.plen, **self.scores, stable_prefix=self.stable_prefix,
                       stable_frame=self.stable_frame, stable_len=self.stable_len, status=status)
        if raw:
            return tensors
        hip.check_prefix_beam_status(status[0], "PrefixBeamStream.push")       # the read drains the stream
        stable = self.stable()
        res = []
        if wrote:
            plen = self.plen.cpu().numpy()
            width = max(int(plen.max()), 1)
            pre, frm = self.prefixes[:, :, :width].cpu().numpy(), self.frames[:, :, :width].cpu().numpy()
            sc = [self.scores[k].cpu().numpy() for k in hip.SCORES]
        for b in range(self.B):
            nbest, frames = [], []
            if wrote:
                for i in range(self.beam):
                    n = int(plen[b, i])
                    if n < 0:
                        continue
                    nbest.append((tuple(pre[b, i, :n].tolist()), *(float(s[b, i]) for s in sc)))
                    frames.append(frm[b, i, :n].tolist())
            res.append({"nbest": nbest, "frames": frames, "stable": stable[b]})
        return res

    def stable(self):
        """Per recording (tokens, frames) of the stable prefix: what every live prefix begins with, final from now on."""
        n = self.stable_len.cpu().tolist()
        width = max(n + [1])
        tok, frm = self.stable_prefix[:, :width].cpu().numpy(), self.stable_frame[:, :width].cpu().numpy()
        return [(tok[b, : n[b]].tolist(), frm[b, : n[b]].tolist()) for b in range(self.B)]
