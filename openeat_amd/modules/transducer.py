"""Transducer (RNN-T) head: a stateless predictor (Ghodsi et al. 2020), the joint network and the transducer loss
(Graves 2012) over an encoder's output, and time-synchronous greedy search.  The reference has no transducer; the loss and
the joint's broadcast are HIP kernels (ops.rnnt_loss, ops.joint_combine; semantics in include/openeat_hip.h)."""
import torch

from openeat_amd import ops


class TransducerHead(torch.nn.Module):
    def __init__(self, vocab_size: int, encoder_dim: int, joint_dim: int = 256, context_size: int = 2, blank: int = 0,
                 activation: str = "tanh", length_normalized_loss: bool = False):
        super().__init__()
        if not (vocab_size >= 2 and 0 <= blank < vocab_size and context_size >= 1):
            raise ValueError(f"TransducerHead: vocab_size={vocab_size} blank={blank} context_size={context_size}")
        self.vocab_size, self.joint_dim, self.context_size, self.blank = vocab_size, joint_dim, context_size, blank
        self.act = ops.ACT_IDS[activation]
        self.length_normalized_loss = bool(length_normalized_loss)
        self.embed = torch.nn.Embedding(vocab_size, joint_dim)
        self.pred = torch.nn.Linear(context_size * joint_dim, joint_dim)
        self.enc_proj = torch.nn.Linear(encoder_dim, joint_dim)
        self.pred_proj = torch.nn.Linear(joint_dim, joint_dim, bias=False)
        self.out = torch.nn.Linear(joint_dim, vocab_size)

    # ------------------------------------------------------------------ parts --
    def predictor(self, ctx: torch.Tensor) -> torch.Tensor:
        """ctx (..., context_size) int64, the last emitted tokens (blank before the start) -> (..., joint_dim)."""
        emb = self.embed.weight[ctx]                                          # a plain table gather
        x = emb.reshape(*ctx.shape[:-1], self.context_size * self.joint_dim)
        return ops.linear(x, self.pred.weight, self.pred.bias, self.act)

    def contexts(self, ys_pad: torch.Tensor, ys_lens: torch.Tensor) -> torch.Tensor:
        """ys_pad (B, U) -> (B, U+1, context_size): position u sees y_{u-context+1} .. y_u, blank before the start and for
        padding (whatever lies at or behind ys_lens is never used as an index)."""
        B, U = ys_pad.shape
        ys = ys_pad.to(torch.int64)
        inside = torch.arange(U, device=ys.device)[None, :] < ys_lens.to(torch.int64)[:, None]
        ys = torch.where(inside & (ys >= 0) & (ys < self.vocab_size), ys, torch.full_like(ys, self.blank))
        padded = torch.cat([torch.full((B, self.context_size), self.blank, dtype=torch.int64, device=ys.device), ys], dim=1)
        return padded.unfold(1, self.context_size, 1)[:, :U + 1]

    def joint_logits(self, encoder_out, ys_pad, encoder_out_lens=None, ys_lens=None):
        """(B, T, D), (B, U) -> raw logits (B, T, U+1, V); nodes outside an utterance's lattice carry the output bias only."""
        if ys_lens is None:
            ys_lens = torch.full((ys_pad.shape[0],), ys_pad.shape[1], dtype=torch.int64, device=ys_pad.device)
        e = ops.linear(encoder_out, self.enc_proj.weight, self.enc_proj.bias)
        p = ops.linear(self.predictor(self.contexts(ys_pad, ys_lens)), self.pred_proj.weight)
        z = ops.joint_combine(e, p, encoder_out_lens, ys_lens, self.act)
        return ops.linear(z, self.out.weight, self.out.bias)

    # ------------------------------------------------------------------ train --
    def logp(self, encoder_out, encoder_out_lens, ys_pad, ys_lens):
        """The transducer log-likelihood of each utterance (B), differentiable; the logits are consumed by the backward."""
        logits = self.joint_logits(encoder_out, ys_pad, encoder_out_lens, ys_lens)
        return ops.rnnt_loss(logits, encoder_out_lens, ys_pad, ys_lens, self.blank, inplace=True)

    def loss_from_logp(self, logp, ys_lens):
        feasible = torch.isfinite(logp.detach())
        total = -torch.where(feasible, logp, torch.zeros_like(logp)).sum()
        if self.length_normalized_loss:
            return total / (ys_lens.to(logp.dtype) * feasible).sum().clamp(min=1.0)
        return total / logp.shape[0]

    def forward(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, ys_pad: torch.Tensor, ys_lens: torch.Tensor):
        """-sum_b logp[b] / B over the feasible utterances (an utterance with no frames, or with a blank or out-of-range target,
        takes no part), or / the number of their labels with length_normalized_loss."""
        return self.loss_from_logp(self.logp(encoder_out, encoder_out_lens, ys_pad, ys_lens), ys_lens)

    # ------------------------------------------------------------------ decode --
    @torch.no_grad()
    def greedy_search(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, max_symbols_per_frame: int = 3):
        """Time-synchronous greedy search over the batch: per frame up to max_symbols_per_frame rounds of predictor -> joint
        for that frame -> top-1; an utterance emits while its best token is not blank, otherwise it moves to the next frame.
        -> tokens (B, Lmax) int32, lens (B) int32, frames (B, Lmax) int32 (the frame of each token), Lmax = T *
        max_symbols_per_frame, all on the device; no host read."""
        B, T, _ = encoder_out.shape
        msf = int(max_symbols_per_frame)
        if msf < 1:
            raise ValueError(f"greedy_search: max_symbols_per_frame={max_symbols_per_frame} < 1")
        dev = encoder_out.device
        e = ops.linear(encoder_out, self.enc_proj.weight, self.enc_proj.bias)
        Lmax = T * msf
        tokens = torch.zeros(B, Lmax, dtype=torch.int32, device=dev)
        frames = torch.zeros(B, Lmax, dtype=torch.int32, device=dev)
        n = torch.zeros(B, dtype=torch.int64, device=dev)
        ctx = torch.full((B, self.context_size), self.blank, dtype=torch.int64, device=dev)
        lens = encoder_out_lens.to(torch.int64)
        rows = torch.arange(B, device=dev)
        for t in range(T):
            emitting = lens > t
            et = e[:, t].contiguous().view(B, 1, self.joint_dim)
            for _ in range(msf):
                p = ops.linear(self.predictor(ctx), self.pred_proj.weight).view(B, 1, self.joint_dim)
                z = ops.joint_combine(et, p, None, None, self.act).view(B, self.joint_dim)
                _, idx = ops.topk_rows(ops.linear(z, self.out.weight, self.out.bias), 1)
                k = idx[:, 0]
                emitting = emitting & (k != self.blank)
                pos = n.clamp(max=Lmax - 1)
                tokens[rows, pos] = torch.where(emitting, k.to(torch.int32), tokens[rows, pos])
                frames[rows, pos] = torch.where(emitting, torch.full_like(frames[rows, pos], t), frames[rows, pos])
                n = n + emitting
                ctx = torch.where(emitting[:, None], torch.cat([ctx[:, 1:], k[:, None]], dim=1), ctx)
        return tokens, n.to(torch.int32), frames
