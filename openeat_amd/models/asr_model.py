"""CTC / attention hybrid ASR model with the reference's public surface
(/root/reference/openeat/models/asr_model.py): constructor kwargs = YAML
``model_conf`` keys, ``forward(features, features_length, targets,
targets_length) -> (loss, acc)``, the four decoding entry points, and the same
flat state-dict keys.  All tensor arithmetic runs in the gfx950 kernels."""
from collections import defaultdict
import math
import os
from typing import List, Optional, Tuple

import torch

from openeat_amd import hip, ops
from openeat_amd import planes as _planes
from openeat_amd.models.ngram_lm import NgramLM
from openeat_amd.modules.cmvn import GlobalCMVN
from openeat_amd.modules.ctc import CTC
from openeat_amd.modules.decoder import BiTransformerDecoder
from openeat_amd.modules.encoder import TransformerEncoder
from openeat_amd.modules.label_smoothing_loss import LabelSmoothingLoss
from openeat_amd.utils.align import frame_times
from openeat_amd.utils.cmvn import load_cmvn
from openeat_amd.utils.common import (IGNORE_ID, add_sos_eos, log_add, remove_duplicates_and_blank, reverse_pad_list)
from openeat_amd.utils.mask import make_pad_mask, mask_finished_preds, mask_finished_scores, subsequent_mask


# The CTC prefix recursion on the device (beam.hip, one wave per utterance); 0: the native host implementation
# (beam_host.cpp, same algorithm, the device kernel's checker).
DEVICE_BEAM = os.environ.get("OE_DEVICE_BEAM", "1") != "0"
DECODE_GRAPHS = os.environ.get("OE_DECODE_GRAPHS", "0") == "1"
DECODE_GRAPH_SLOTS = 8
EDIT_DISTANCE_MAX = 1023                                                     # oe_edit_distance: columns per sequence
ATT_INPUTS_KERNEL = os.environ.get("OE_ATT_INPUTS_KERNEL", "1") != "0"      # decoder token bookkeeping as one launch (fixed widths)


def _device_beam(beam_size):
    """Whether the plain prefix recursion of this beam runs on the device (DEVICE_BEAM is read at the time of the call)."""
    return DEVICE_BEAM and beam_size <= 16


def _graph_call(cache, key, fn, args):
    """fn(*args) through a per-key HIP graph: first call eager (lazy state must exist before a capture) and captured for
    the next time, later calls copy the arguments into the capture's static inputs and replay.  Outputs are the capture's
    own tensors (valid until the next replay of the same key).  A key whose capture failed stays eager.  None stays None."""
    rec = cache.get(key, False)
    if rec is None:
        return fn(*args)
    if rec is False:
        out = fn(*args)                                            # the real result of this call
        static = tuple(None if a is None else a.clone() for a in args)
        g = torch.cuda.CUDAGraph()
        try:
            torch.cuda.synchronize()
            # the capture neither reads pre-split operands that eager code made (the registry's FIFO would free them under the
            # graph: the position table's planes, round 3's red replay) nor leaves its own - unwritten until the first replay - behind
            with _planes.capture_scope(), torch.cuda.graph(g):
                sout = fn(*static)
            cache[key] = (g, static, sout)
        except Exception as e:                                     # noqa: BLE001 - whatever the capture objected to: stay eager
            import warnings
            warnings.warn(f"decode stage {key[0]} {key[1]} is not capturable ({type(e).__name__}: {str(e)[:200]}); it keeps running eagerly")
            cache[key] = None
        stage = [k for k in cache if k[0] == key[0]]
        for k in stage[:-DECODE_GRAPH_SLOTS]:
            del cache[k]
        return out
    g, static, sout = rec
    for s_, a in zip(static, args):
        if a is not None:
            s_.copy_(a)
    g.replay()
    return sout


class ASRModel(torch.nn.Module):
    def __init__(self, input_size: int, vocab_size: int, is_json_cmvn: bool = True, cmvn_file: str = None,
                 cn_cmvn_file: str = None, en_cmvn_file: str = None, encoder_num_blocks: int = 12,
                 encoder_num_blocks_share: int = 1, decoder_num_blocks: int = 6, r_decoder_num_blocks: int = 0,
                 decoder_num_blocks_share: int = 1, input_layer: str = "conv2d", pos_enc_layer_type: str = "rel_pos",
                 d_model: int = 256, attention_heads: int = 4, linear_units: int = 1024, dropout_rate: float = 0.1,
                 activation_type: str = "swish", macaron_style: bool = True, use_cnn_module: bool = True,
                 cnn_module_kernel: int = 15, causal: bool = False, encoder_use_adapter: bool = False,
                 decoder_use_adapter: bool = False, down_size: int = 64, scalar: float = 0.1, ctc_weight: float = 0.3,
                 lsm_weight: float = 0.1, reverse_weight: float = 0.0, length_normalized_loss: bool = False,
                 ignore_id=IGNORE_ID):
        super().__init__()
        self.input_size = input_size
        self.vocab_size = vocab_size
        self.sos = vocab_size - 1
        self.eos = vocab_size - 1
        self.ignore_id = ignore_id
        self.ctc_weight = ctc_weight
        self.reverse_weight = reverse_weight
        global_cmvn = None
        if cmvn_file is not None:
            mean, istd = load_cmvn(cmvn_file, is_json_cmvn)
            global_cmvn = GlobalCMVN(torch.from_numpy(mean).float(), torch.from_numpy(istd).float())
        self.encoder = TransformerEncoder(
            input_size, input_layer, pos_enc_layer_type, d_model, dropout_rate, attention_heads, linear_units,
            activation_type, macaron_style, use_cnn_module, cnn_module_kernel, causal, encoder_use_adapter, down_size,
            scalar, num_blocks=encoder_num_blocks, num_blocks_share=encoder_num_blocks_share, global_cmvn=global_cmvn)
        self.ctc = CTC(vocab_size, d_model, length_normalized_loss)
        self.decoder = BiTransformerDecoder(
            vocab_size, d_model, dropout_rate, attention_heads, linear_units, decoder_use_adapter, down_size, scalar,
            num_blocks=decoder_num_blocks, r_num_blocks=r_decoder_num_blocks, num_blocks_share=decoder_num_blocks_share)
        self.criterion_att = LabelSmoothingLoss(size=vocab_size, padding_idx=ignore_id, smoothing=lsm_weight,
                                                normalize_length=length_normalized_loss)

    # ------------------------------------------------------------------ train --
    def _encode(self, features, features_length):
        _planes.new_pass()                      # (decode entry points come through here without forward()'s predrop_clear)
        masks = ~make_pad_mask(features_length, features.size(1)).unsqueeze(1)      # (B,1,T)
        return self.encoder(features, masks)

    def forward(self, features: torch.Tensor, features_length: torch.Tensor, targets: torch.Tensor,
                targets_length: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """asr_model.py:126-157."""
        assert targets_length.dim() == 1, targets_length.shape
        assert (features.shape[0] == features_length.shape[0] == targets.shape[0] == targets_length.shape[0]), \
            (features.shape, features_length.shape, targets.shape, targets_length.shape)
        ops.predrop_clear()                     # a new tape starts: nothing of the previous backward may be picked up
        par = ops.PARALLEL_DECODERS and features.is_cuda and self.ctc_weight < 1
        prep = None
        if par:
            # the decoders' token bookkeeping (sos/eos, reversal, masks: ~60 tiny launches that depend on the targets only)
            # runs on the decoder stream while the encoder runs here; it is joined where the decoders start
            main, side = torch.cuda.current_stream(), ops.decoder_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                prep = self._att_inputs(targets, targets_length)
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        if par:
            main.wait_stream(side)
            for t in prep:
                if isinstance(t, torch.Tensor):
                    t.record_stream(main)
        ops.stamp("fwd: encoder done")
        ops.stamp_grad(encoder_out, "bwd: heads done")
        hooks = getattr(self, "grad_ready_hooks", None)          # set by TrainEngine for multi-GPU overlap
        if hooks and encoder_out.requires_grad:
            cb = hooks["encoder_out"]
            encoder_out.register_hook(lambda g, cb=cb: cb())      # returns None: the gradient is not modified
            encoder_out = ops.cut(encoder_out, "heads")           # segmented capture: the tape ends here (identity otherwise)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        if par:
            # the CTC head (a few chip-filling launches) on a third stream beside the decoders' latency-bound chains
            main, side = torch.cuda.current_stream(), ops.ctc_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                ops.stamp("fwd: ctc head starts (its stream)")
                loss_ctc = self.ctc(encoder_out, encoder_out_lens, targets, targets_length)
                ops.stamp("fwd: ctc head done (its stream)")
            l_loss, r_loss, acc = self._att_losses(encoder_out, encoder_mask, targets, targets_length, prep)
            main.wait_stream(side)
            loss_ctc.record_stream(main)
            return self._joint_loss(loss_ctc, l_loss, r_loss), acc
        loss_ctc = self.ctc(encoder_out, encoder_out_lens, targets, targets_length)
        if self.ctc_weight < 1:
            l_loss, r_loss, acc = self._att_losses(encoder_out, encoder_mask, targets, targets_length)
            return self._joint_loss(loss_ctc, l_loss, r_loss), acc
        return loss_ctc, None

    def forward_mwer(self, features: torch.Tensor, features_length: torch.Tensor, targets: torch.Tensor, targets_length: torch.Tensor,
                     nbest: int = 4, ce_weight: float = 0.01, nbest_lists=None):
        """Minimum word error rate training step over the model's own n-best lists (Prabhavalkar et al. 2018; the reference
        trains on likelihood only).  One encoder pass; without gradient the device prefix beam search (`nbest` entries per
        utterance) on the CTC logits and every entry's error count against the transcript; then the entries' exact CTC
        log-likelihoods (ops.ctc_nbest_logp, differentiable), renormalised over the list:
            loss = mean_b sum_n P_n (W_n - mean W) + ce_weight * (the joint loss of forward()).
        Entries that do not exist or have no alignment (logp = -inf) take no part.  Eager only; no host read.
        nbest_lists: (prefixes (B * nbest, T') int, lengths (B * nbest) int) to score instead of searching.
        -> loss, info: device tensors loss_mwer, loss_base, acc (None with ctc_weight == 1), expected_errors (B), logp (B, nbest),
        errors (B, nbest), prefixes (B * nbest, T') int32, plen (B * nbest) int32.  Needs the device beam and nbest <= 16
        (ValueError otherwise: there is no host implementation)."""
        from openeat_amd.utils.mwer import mwer_loss
        assert targets_length.dim() == 1, targets_length.shape
        assert (features.shape[0] == features_length.shape[0] == targets.shape[0] == targets_length.shape[0]), \
            (features.shape, features_length.shape, targets.shape, targets_length.shape)
        spec = hip.PrefixSearch(int(nbest))
        spec.validate("forward_mwer", DEVICE_BEAM)
        nbest = spec.beam
        ops.predrop_clear()
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        logits = self.ctc.logits(encoder_out)
        B, T = logits.shape[0], logits.shape[1]
        with torch.no_grad():
            if nbest_lists is None:
                top_p, top_i = ops.topk_rows(logits.detach(), nbest, log_softmax=True)
                r = hip._prefix_beam_device("forward_mwer", top_p, top_i, encoder_out_lens.to(torch.int32), spec, True)
                prefixes, plen = r.prefixes.view(B * nbest, -1), r.plen.view(B * nbest)
            else:
                prefixes, plen = nbest_lists
            counts = ops.edit_distance(targets, targets_length, prefixes[:, :EDIT_DISTANCE_MAX], plen, group=nbest)
            errors = counts[:, 1:].sum(1).view(B, nbest)
        logp = ops.ctc_nbest_logp(logits, encoder_out_lens, prefixes[:, :min(T, 255)], plen, nbest)
        exists = torch.isfinite(logp.detach())
        per_utt, expected = mwer_loss(logp, errors.to(logp.dtype), exists)
        loss_mwer = per_utt.mean()
        loss_ctc = self.ctc(encoder_out, encoder_out_lens, targets, targets_length)
        acc = None
        if self.ctc_weight < 1:
            l_loss, r_loss, acc = self._att_losses(encoder_out, encoder_mask, targets, targets_length)
            base = self._joint_loss(loss_ctc, l_loss, r_loss)
        else:
            base = loss_ctc
        loss = loss_mwer + ce_weight * base
        return loss, dict(loss_mwer=loss_mwer.detach(), loss_base=base.detach(), acc=acc, expected_errors=expected.detach(),
                          logp=logp.detach(), errors=errors, prefixes=prefixes, plen=plen)

    # ------------------------------------------------------------------ transducer --
    def add_transducer(self, **head_conf):
        """Give the model a transducer head over its encoder (modules/transducer.py; the reference has none): head_conf are
        TransducerHead's keyword arguments (joint_dim, context_size, blank, activation, length_normalized_loss).  A model
        without the head keeps exactly the state dict it had; with it the keys transducer.* are added."""
        from openeat_amd.modules.transducer import TransducerHead
        d_model = self.ctc.ctc_lo.in_features
        self.transducer = TransducerHead(self.vocab_size, d_model, **head_conf).to(self.ctc.ctc_lo.weight.device)
        return self.transducer

    def _transducer_head(self, who):
        head = getattr(self, "transducer", None)
        if head is None:
            raise RuntimeError(f"{who}: the model has no transducer head; call add_transducer() first")
        return head

    def forward_transducer(self, features: torch.Tensor, features_length: torch.Tensor, targets: torch.Tensor,
                           targets_length: torch.Tensor, rnnt_weight: float = 1.0, base_weight: float = 0.0):
        """Transducer training step: one encoder pass, then
            loss = rnnt_weight * (the head's loss, -sum_b logp[b] / B) + base_weight * (the joint CTC/attention loss of forward()).
        The base loss is not computed with base_weight == 0.  Eager only; no host read.
        -> loss, info: device tensors logp (B), loss_rnnt, loss_base (None with base_weight == 0), acc (None unless the
        attention decoder ran)."""
        head = self._transducer_head("forward_transducer")
        assert targets_length.dim() == 1, targets_length.shape
        assert (features.shape[0] == features_length.shape[0] == targets.shape[0] == targets_length.shape[0]), \
            (features.shape, features_length.shape, targets.shape, targets_length.shape)
        ops.predrop_clear()
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        logp = head.logp(encoder_out, encoder_out_lens, targets, targets_length)
        loss_rnnt = head.loss_from_logp(logp, targets_length)
        loss, base, acc = rnnt_weight * loss_rnnt, None, None
        if base_weight != 0:
            loss_ctc = self.ctc(encoder_out, encoder_out_lens, targets, targets_length)
            if self.ctc_weight < 1:
                l_loss, r_loss, acc = self._att_losses(encoder_out, encoder_mask, targets, targets_length)
                base = self._joint_loss(loss_ctc, l_loss, r_loss)
            else:
                base = loss_ctc
            loss = loss + base_weight * base
        return loss, dict(logp=logp.detach(), loss_rnnt=loss_rnnt.detach(), loss_base=None if base is None else base.detach(), acc=acc)

    def transducer_greedy_search(self, features: torch.Tensor, features_length: torch.Tensor,
                                 max_symbols_per_frame: int = 3) -> List[List[int]]:
        """Greedy transducer decoding (TransducerHead.greedy_search) -> the token list of each utterance.  The search runs on
        the device; the tokens come to the host once, at the end."""
        head = self._transducer_head("transducer_greedy_search")
        with torch.no_grad():
            encoder_out, encoder_mask, _ = self._encode(features, features_length)
            tokens, lens, _ = head.greedy_search(encoder_out, encoder_mask.squeeze(1).sum(1), max_symbols_per_frame)
        tokens, lens = tokens.cpu().tolist(), lens.cpu().tolist()
        return [row[:n] for row, n in zip(tokens, lens)]

    def ctc_graph_loss(self, features: torch.Tensor, features_length: torch.Tensor, graphs, graph_of=None,
                       targets: Optional[torch.Tensor] = None, targets_length: Optional[torch.Tensor] = None,
                       denominator=None, den_beam: float = 12.0, den_scale: float = 1.0, den_max_active: Optional[int] = None):
        """Training against decoding graphs (what k2 / WeNet users know as a graph CTC loss; the reference trains on one
        spelling only): `graphs` a DecodingGraph, a list of them or a GraphSet (openeat_amd.utils.decoding_graph; transcripts
        with alternatives come from DecodingGraph.from_alternatives), graph_of (B) the graph of each utterance (None: graph 0
        for all).  One encoder pass; logp = ops.ctc_graph_logp on the CTC logits (semantics in include/openeat_hip.h,
        oe_ctc_graph_logp), and loss_ctc = -(the sum of logp over the feasible utterances) / B, the zero_infinity convention
        of the CTC head.  With `targets` (the canonical spelling) and ctc_weight < 1 the attention losses are computed on
        them and combined as in forward(); otherwise the result is the CTC term alone.  Eager only; no host read.
        denominator (a DecodingGraph of any size; MMI-style training): logp_den = ops.ctc_graph_beam_logp over that one graph
        with beam den_beam and max_active den_max_active (default 16384; semantics at oe_ctc_graph_beam_logp), and loss_ctc =
        -(the sum over the feasible utterances of logp - den_scale * logp_den) / B, feasible meaning both terms are finite.
        This path reads the denominator's status and peak on the host, one D2H copy per round, to run overflowed utterances
        again with max_active doubled (one copy when nothing overflows); `info` gains logp_den.
        -> loss, info: device tensors logp (B), feasible (B) bool, acc (None without the attention term)."""
        assert features.shape[0] == features_length.shape[0]
        ops.predrop_clear()
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        logits = self.ctc.logits(encoder_out)
        logp = ops.ctc_graph_logp(logits, encoder_out_lens, graphs, graph_of)
        feasible = torch.isfinite(logp.detach())
        logp_den = None
        if denominator is not None:
            logp_den = self._graph_beam_logp(logits, encoder_out_lens, denominator, float(den_beam),
                                             16384 if den_max_active is None else int(den_max_active), 1 << 30)[0]
            feasible = feasible & torch.isfinite(logp_den.detach())
            term = logp - float(den_scale) * logp_den
        else:
            term = logp
        loss_ctc = -torch.where(feasible, term, torch.zeros_like(logp)).sum() / logp.shape[0]
        acc = None
        loss = loss_ctc
        if targets is not None and self.ctc_weight < 1:
            assert targets_length is not None and targets.shape[0] == targets_length.shape[0] == features.shape[0]
            l_loss, r_loss, acc = self._att_losses(encoder_out, encoder_mask, targets, targets_length)
            loss = self._joint_loss(loss_ctc, l_loss, r_loss)
        info = dict(logp=logp.detach(), feasible=feasible, acc=acc)
        if logp_den is not None:
            info["logp_den"] = logp_den.detach()
        return loss, info

    @torch.no_grad()
    def ctc_nbest(self, features: torch.Tensor, features_length: torch.Tensor, beam_size: int):
        """The CTC n-best list of every utterance with each entry's EXACT CTC log-likelihood beside the beam's score (which
        sums only the alignments that survived the pruning, so exact >= beam up to rounding): per utterance
        [(tokens tuple, beam_score, exact_logp)] in the beam's order.  Device beam only (ValueError otherwise)."""
        assert features.shape[0] == features_length.shape[0]
        spec = hip.PrefixSearch(int(beam_size))
        spec.validate("ctc_nbest", DEVICE_BEAM)
        encoder_out, encoder_mask, pre, plen, scores, bad, _ = self._rescore_stage1(features, features_length, spec)
        B, T = encoder_out.shape[0], encoder_out.shape[1]
        exact = ops.ctc_nbest_logp(self.ctc.logits(encoder_out), encoder_mask.squeeze(1).sum(1), pre[:, :min(T, 255)], plen, spec.beam)
        lists = hip._nbest_lists(pre.view(B, spec.beam, -1), plen.view(B, spec.beam), scores.view(B, spec.beam), exact)
        hip.check_prefix_beam_status(bad, "ctc_nbest")            # (the copies above have drained the stream)
        return lists

    def _joint_loss(self, loss_ctc, l_loss, r_loss):
        """asr_model.py:150-157 with :196-198 folded in: ctc_weight * ctc + (1 - ctc_weight) * (l * (1 - rw) + r * rw)."""
        if l_loss.is_cuda and l_loss.dtype == torch.float32:
            return ops.combine_losses(l_loss, r_loss, loss_ctc, self.ctc_weight, self.reverse_weight)
        loss_att = l_loss if r_loss is None else l_loss * (1 - self.reverse_weight) + r_loss * self.reverse_weight
        return self.ctc_weight * loss_ctc + (1 - self.ctc_weight) * loss_att

    def _att_inputs(self, ys_pad, ys_pad_lens):
        """asr_model.py:162-176: decoder inputs / targets of both directions and the target mask (token bookkeeping only)."""
        from openeat_amd.utils import common
        if ATT_INPUTS_KERNEL and common.STATIC_SHAPES and ys_pad.is_cuda and ys_pad.dtype == torch.int32 and ys_pad_lens.dtype == torch.int32 \
                and ys_pad.dim() == 2 and ys_pad.shape[1] <= 8000:
            # fixed width (a captured step): one launch instead of ~70 index-arithmetic launches
            B, L = ys_pad.shape
            W = L + 1
            rev = self.reverse_weight > 0
            out = torch.empty(4 if rev else 2, B, W, dtype=torch.long, device=ys_pad.device)
            tgt_mask = torch.empty(B, W, W, dtype=torch.bool, device=ys_pad.device)
            hip.call("oe_att_inputs", ys_pad.contiguous(), ys_pad_lens.contiguous(), B, L, self.sos, self.eos, self.ignore_id, out[0], out[1],
                     out[2] if rev else None, out[3] if rev else None, tgt_mask)
            return out[0], out[1], tgt_mask, (out[2] if rev else None), (out[3] if rev else None)
        ys_in_pad, ys_out_pad = add_sos_eos(ys_pad, self.sos, self.eos, self.ignore_id)
        ys_in_lens = ys_pad_lens + 1
        L = ys_in_pad.size(1)
        tgt_mask = (~make_pad_mask(ys_in_lens, L)).unsqueeze(1) & subsequent_mask(L, device=ys_in_pad.device).unsqueeze(0)
        r_ys_in_pad = r_ys_out_pad = None
        if self.reverse_weight > 0:
            r_ys_pad = reverse_pad_list(ys_pad, ys_pad_lens, float(self.ignore_id))
            r_ys_in_pad, r_ys_out_pad = add_sos_eos(r_ys_pad, self.sos, self.eos, self.ignore_id)
        return ys_in_pad, ys_out_pad, tgt_mask, r_ys_in_pad, r_ys_out_pad

    def _calc_att_loss(self, encoder_out, encoder_mask, ys_pad, ys_pad_lens, prep=None):
        """asr_model.py:159-203; the output layers are fused with the loss."""
        l_loss, r_loss, acc = self._att_losses(encoder_out, encoder_mask, ys_pad, ys_pad_lens, prep)
        if r_loss is None:
            return l_loss, acc
        if l_loss.is_cuda and l_loss.dtype == torch.float32:
            return ops.combine_losses(l_loss, r_loss, None, 0.0, self.reverse_weight), acc
        return l_loss * (1 - self.reverse_weight) + r_loss * self.reverse_weight, acc

    def _att_losses(self, encoder_out, encoder_mask, ys_pad, ys_pad_lens, prep=None):
        """The two decoders' losses of asr_model.py:159-203 before they are mixed: (left, right or None, accuracy)."""
        ys_in_pad, ys_out_pad, tgt_mask, r_ys_in_pad, r_ys_out_pad = prep if prep is not None else self._att_inputs(ys_pad, ys_pad_lens)
        dec = self.decoder

        def left():
            l_hid = dec.left_decoder.hidden(ys_in_pad, tgt_mask, encoder_out, encoder_mask)
            lo = dec.left_decoder.output_layer
            return self.criterion_att.fused_head(l_hid, lo.weight, lo.bias, ys_out_pad)

        if not self.reverse_weight > 0:
            loss_att, n_ok, n_valid = left()
            return loss_att, None, torch.true_divide(n_ok, n_valid)

        def right():
            r_hid = dec.right_decoder.hidden(r_ys_in_pad, tgt_mask, encoder_out, encoder_mask)
            ro = dec.right_decoder.output_layer
            return self.criterion_att.fused_head(r_hid, ro.weight, ro.bias, r_ys_out_pad)[0]

        if ops.PARALLEL_DECODERS and encoder_out.is_cuda:
            # the right decoder on its own stream beside the left one (ops.PARALLEL_DECODERS): fork here, join below
            main, side = torch.cuda.current_stream(), ops.decoder_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                ops.stamp("fwd: right decoder starts (its stream)")
                r_loss = right()
                ops.stamp("fwd: right decoder done (its stream)")
            ops.stamp("fwd: left decoder starts")
            loss_att, n_ok, n_valid = left()
            ops.stamp("fwd: left decoder done")
            main.wait_stream(side)
            r_loss.record_stream(main)
        else:
            loss_att, n_ok, n_valid = left()
            r_loss = right()
        return loss_att, r_loss, torch.true_divide(n_ok, n_valid)

    # ----------------------------------------------------------------- decode --
    def _ctc_greedy(self, features, features_length):
        """asr_model.py:297-326 on the device: argmax / eos-fill / collapse -> tokens (B, T') and their counts (B)."""
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        lens = encoder_mask.squeeze(1).sum(1)
        logits = self.ctc.logits(encoder_out)
        B, T, V = logits.shape
        return ops.ctc_greedy(logits, V, B, T, V, lens, self.eos)

    def _ctc_topk(self, features, features_length, beam_size):
        """What every prefix search starts from: one encoder pass, the valid encoder frames (B) int32 and the fused log-softmax
        top-k of the CTC logits -> encoder_out, encoder_mask, lens, top_p (B, T', beam) float32, top_i (B, T', beam) int64."""
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        lens = encoder_mask.squeeze(1).sum(1).to(torch.int32)
        top_p, top_i = ops.topk_rows(self.ctc.logits(encoder_out), beam_size, log_softmax=True)
        return encoder_out, encoder_mask, lens, top_p, top_i

    def _span_logits(self, features, features_length, spans):
        """spans: [(recording, f0, f1)], feature frames f0..f1 of a recording -> the CTC logits (len(spans), T', V) of the spans
        encoded as ONE batch, zero-padded to the longest."""
        flen = torch.tensor([f1 - f0 for _, f0, f1 in spans], dtype=features_length.dtype, device=features.device)
        batch = features.new_zeros(len(spans), int(flen.max()), features.shape[2])
        for w, (b, f0, f1) in enumerate(spans):
            batch[w, : f1 - f0] = features[b, f0:f1]
        encoder_out, _, _ = self._encode(batch, flen)
        return self.ctc.logits(encoder_out)

    def ctc_greedy_search(self, features: torch.Tensor, features_length: torch.Tensor) -> List[List[int]]:
        """asr_model.py:297-326: argmax / eos-fill / collapse all on device; one D2H copy of the result."""
        assert features.shape[0] == features_length.shape[0]
        toks, n = self._ctc_greedy(features, features_length)
        toks, n = toks.cpu(), n.cpu()
        return [toks[b, : int(n[b])].tolist() for b in range(len(n))]

    @torch.no_grad()
    def ctc_align(self, features: torch.Tensor, features_length: torch.Tensor, targets: torch.Tensor,
                  targets_length: torch.Tensor, with_times: bool = False, frame_shift_ms: float = 10):
        """CTC forced alignment of each utterance to its own target (the reference has none; semantics in
        include/openeat_hip.h): recursion and back-trace on the device, one D2H copy of the results.  Per utterance a dict
        `frames` (token id of every valid encoder frame, 0 = blank), `tokens` (one dict per label: `token`, `start_frame`,
        `end_frame` (inclusive), `confidence` = exp(mean log-prob over the span), and with_times `start_s` / `end_s`),
        `score` (log-prob of the path); None for an utterance whose target does not fit its frames."""
        assert features.shape[0] == features_length.shape[0] == targets.shape[0] == targets_length.shape[0]
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        lens = encoder_mask.squeeze(1).sum(1)
        frames, start, end, logp, score = self.ctc.forced_align(encoder_out, lens, targets, targets_length)
        B, T = frames.shape
        Lmax = start.shape[1]
        cols = [frames, start, end, logp, targets[:, :Lmax], score.unsqueeze(1), lens.unsqueeze(1), targets_length.unsqueeze(1)]
        packed = torch.cat([c.double() for c in cols], dim=1).cpu()          # (int32 and float32 are exact in float64)
        frames, start, end, logp, targets = (packed[:, :T].long(), packed[:, T:T + Lmax].long(), packed[:, T + Lmax:T + 2 * Lmax].long(),
                                             packed[:, T + 2 * Lmax:T + 3 * Lmax], packed[:, T + 3 * Lmax:T + 4 * Lmax].long())
        score, lens, targets_length = packed[:, -3], packed[:, -2].long(), packed[:, -1].long()
        rate = self.encoder.embed.subsampling_rate
        out = []
        for b in range(B):
            if score[b] == float("-inf"):
                out.append(None)
                continue
            toks = []
            for l in range(int(targets_length[b])):
                s, e = int(start[b, l]), int(end[b, l])
                tok = {"token": int(targets[b, l]), "start_frame": s, "end_frame": e,
                       "confidence": math.exp(float(logp[b, l]) / (e - s + 1))}
                if with_times:
                    tok["start_s"], tok["end_s"] = frame_times(s, e, rate, frame_shift_ms)
                toks.append(tok)
            out.append({"frames": frames[b, : int(lens[b])].tolist(), "tokens": toks, "score": float(score[b])})
        return out

    @torch.no_grad()
    def ctc_logits_windowed(self, features: torch.Tensor, features_length: torch.Tensor, window: Optional[int], margin: int = 16):
        """CTC logits of whole recordings, longer than one attention pass holds -> (logits (B, T', V), lens (B)).  Each
        recording is cut by utils.segment.window_plan into kept spans of `window` encoder frames computed with `margin` frames of
        context on either side; the windows of one recording go through _encode and ctc.logits as ONE batch (in plan order,
        zero-padded to the longest), and their kept frames are copied to their place.  window None, or at or above every
        recording's T': one plain pass over the batch."""
        from openeat_amd.utils.segment import encoder_frames, window_plan
        embed = self.encoder.embed
        rate, rc = embed.subsampling_rate, embed.right_context
        n_feats = [int(n) for n in features_length.tolist()]
        n_enc = [encoder_frames(n, rate, rc) for n in n_feats]
        if window is None or window >= max(n_enc):
            encoder_out, encoder_mask, _ = self._encode(features, features_length)
            return self.ctc.logits(encoder_out), encoder_mask.squeeze(1).sum(1)
        out = None
        for b, n in enumerate(n_feats):
            plan = window_plan(n, window, margin, rate, rc)
            lg = self._span_logits(features, features_length, [(b, f0, f1) for f0, f1, _, _, _ in plan])
            if out is None:
                out = lg.new_zeros(len(n_feats), max(n_enc), lg.shape[2])
            for w, (_, _, q0, q1, o0) in enumerate(plan):
                out[b, o0:o0 + q1 - q0] = lg[w, q0:q1]
        return out, torch.tensor(n_enc, dtype=torch.int64, device=features.device)

    @torch.no_grad()
    def ctc_segment(self, features: torch.Tensor, features_length: torch.Tensor, utterances, window: Optional[int] = None,
                    margin: int = 16, free_start: bool = True, free_end: bool = True, score_window: int = 30,
                    with_times: bool = False, frame_shift_ms: float = 10):
        """Long-form CTC segmentation (the reference has none; semantics in include/openeat_hip.h): each recording is aligned to
        the concatenation of its utterances, utterances[b] a list of token-id lists, with the audio before / after the
        transcript free.  Logits by ctc_logits_windowed (window None: one plain pass), recursion and back-trace on the device,
        one D2H copy of the results.  Per recording {"score": log-prob of the path, "utterances": [{"start_frame",
        "end_frame" (inclusive encoder frames), "mean_logp", "min_logp" (utils.segment.segment_stats over score_window frames),
        "confidence" = exp(min_logp), and with_times "start_s" / "end_s"}]}; None for a recording whose transcript does not
        fit its frames."""
        from openeat_amd.utils.segment import segment_stats
        B = features.shape[0]
        assert B == features_length.shape[0] == len(utterances)
        if any(len(u) == 0 for rec in utterances for u in rec) or any(len(rec) == 0 for rec in utterances):
            raise ValueError("ctc_segment: every recording needs utterances and every utterance labels")
        logits, lens = self.ctc_logits_windowed(features, features_length, window, margin)
        dev = logits.device
        offsets = [[0] for _ in range(B)]
        for b, rec in enumerate(utterances):
            for u in rec:
                offsets[b].append(offsets[b][-1] + len(u))
        Lmax = max(o[-1] for o in offsets)
        ys = torch.zeros(B, Lmax, dtype=torch.int64)
        for b, rec in enumerate(utterances):
            ys[b, : offsets[b][-1]] = torch.tensor([t for u in rec for t in u], dtype=torch.int64)
        ylens = torch.tensor([o[-1] for o in offsets], dtype=torch.int32)
        _, T, V = logits.shape
        _, path_logp, start, end, _, score = ops.ctc_segment(logits, V, B, T, V, lens, ys.to(dev), ylens.to(dev), free_start, free_end)
        cols = []
        for b in range(B):
            L = offsets[b][-1]
            st = segment_stats(path_logp[b], start[b, :L], end[b, :L], offsets[b], score_window)
            cols += [score[b:b + 1]] + [c.double() for c in st]
        packed = torch.cat(cols).cpu().tolist()
        rate = self.encoder.embed.subsampling_rate
        out, at = [], 0
        for b in range(B):
            U = len(utterances[b])
            sc, s, e, mean, mn = packed[at], *(packed[at + 1 + i * U: at + 1 + (i + 1) * U] for i in range(4))
            at += 1 + 4 * U
            if sc == float("-inf"):
                out.append(None)
                continue
            segs = []
            for u in range(U):
                seg = {"start_frame": int(s[u]), "end_frame": int(e[u]), "mean_logp": mean[u], "min_logp": mn[u],
                       "confidence": math.exp(mn[u])}
                if with_times:
                    seg["start_s"], seg["end_s"] = frame_times(int(s[u]), int(e[u]), rate, frame_shift_ms)
                segs.append(seg)
            out.append({"score": sc, "utterances": segs})
        return out

    @torch.no_grad()
    def keyword_search(self, features: torch.Tensor, features_length: torch.Tensor, keywords, window: Optional[int] = None,
                       margin: int = 16, max_hits: int = 8, with_times: bool = False, frame_shift_ms: float = 10):
        """Keyword search (spoken-term detection; the reference has none; semantics in include/openeat_hip.h, oe_ctc_kws): where
        each keyword of `keywords`, an openeat_amd.utils.keyword.KeywordList, occurs in each recording - every occurrence whose
        mean posterior per frame reaches the keyword's threshold, not the 1-best's.  Logits by ctc_logits_windowed (window
        None: one plain pass), recursion and hit scan on the device, one D2H copy of the results.  Returns (hits, truncated):
        hits[b] the recording's hits in time order, each {"keyword": index, "tokens", "start_frame", "end_frame" (inclusive
        encoder frames), "score" (log-probability of the hit's path), "confidence" = exp(score / frames), and with_times
        "start_s" / "end_s"}; truncated[b][k]: more than max_hits hits were found and only the first max_hits are listed."""
        from openeat_amd.utils.keyword import KeywordList, hit_records
        if not isinstance(keywords, KeywordList):
            raise ValueError(f"keywords must be an openeat_amd.utils.keyword.KeywordList (got {type(keywords).__name__})")
        assert features.shape[0] == features_length.shape[0]
        logits, lens = self.ctc_logits_windowed(features, features_length, window, margin)
        n_hits, start, end, score = ops.ctc_keyword_search(logits, lens, keywords, max_hits)[:4]
        B, K = n_hits.shape
        packed = torch.cat([n_hits.double().flatten(), start.double().flatten(), end.double().flatten(), score.double().flatten()]).cpu()
        n, s, e, sc = packed[: B * K], *packed[B * K:].split(B * K * max_hits)
        shape = (B, K, max_hits)
        rate = self.encoder.embed.subsampling_rate
        times = (lambda a, b: frame_times(a, b, rate, frame_shift_ms)) if with_times else None
        return hit_records(keywords, n.view(B, K).tolist(), s.view(shape).tolist(), e.view(shape).tolist(), sc.view(shape).tolist(), times)

    @torch.no_grad()
    def ctc_graph_search(self, features: torch.Tensor, features_length: torch.Tensor, graph, window: Optional[int] = None,
                         margin: int = 16, with_times: bool = False, frame_shift_ms: float = 10, posterior: bool = False,
                         beam: Optional[float] = None, max_active: Optional[int] = None, workspace_cap: int = 1 << 30,
                         nbest: Optional[int] = None, distinct: str = "arcs", posterior_beam: Optional[float] = None):
        """Grammar-constrained CTC decoding (the reference has none; semantics in include/openeat_hip.h, oe_ctc_graph): the
        best path of each utterance through `graph`, an openeat_amd.utils.decoding_graph.DecodingGraph - the output is in the
        grammar by construction, or the utterance is infeasible.  Logits by ctc_logits_windowed (window None: one plain pass),
        recursion, back-trace and traversal list on the device, one D2H copy of the results.  Returns a GraphResult per
        utterance (tokens, traversals and outputs with their frame spans, score, feasible; with_times adds seconds).
        posterior=True: each result also carries log_mass, the graph's total log-likelihood on the normalised posteriors
        (ops.ctc_graph_logp: with zero weights log P(the labelling is in the grammar), a rejection score), and posterior =
        exp(score - log_mass), the best path's share of it; one more recursion on the device and one more D2H copy.
        posterior_beam a float >= 0 or inf (with or without posterior=True, with either search): log_mass and posterior come
        from the beam-pruned sum instead (ops.ctc_graph_beam_logp with that beam; semantics at oe_ctc_graph_beam_logp), which
        takes a graph of any size; an utterance that overflows max_active is run again with it doubled, as the beam search's.
        beam None: the dense search (oe_ctc_graph; graphs of at most 8064 nodes and 16384 arcs).  beam a float >= 0 or inf:
        the token-passing search (oe_ctc_graph_beam), the one a large=True graph has: after every frame but the last the
        states below the frame's best - beam are dropped, and max_active (default 16384) is how many survivors a frame can
        record.  An utterance that overflows is run again, alone with the others that did, with max_active doubled (and at
        least its peak), for as long as one utterance's workspace stays within workspace_cap; after that a RuntimeError names the
        utterance and its peak.  An utterance may be infeasible through pruning alone; a wider beam is the remedy.
        nbest = K (1 .. 8; dense search only, a ValueError with beam): every result also carries .nbest, the K best distinct
        paths (distinct="arcs") or token sequences (distinct="tokens") as GraphHypothesis, best first (ops.ctc_graph_nbest,
        semantics at oe_ctc_graph_nbest): one more pass on the device and one more D2H copy.  nbest[0] is the 1-best's path."""
        from openeat_amd.utils.decoding_graph import LOGP_MAX_ARCS, LOGP_MAX_NODES, DecodingGraph, graph_results
        if not isinstance(graph, DecodingGraph):
            raise ValueError(f"graph must be an openeat_amd.utils.decoding_graph.DecodingGraph (got {type(graph).__name__})")
        if posterior and posterior_beam is None and (graph.num_nodes > LOGP_MAX_NODES or graph.num_arcs > LOGP_MAX_ARCS):
            raise ValueError(f"posterior=True needs the graph's total likelihood (oe_ctc_graph_logp), which takes at most {LOGP_MAX_NODES} "
                             f"nodes and {LOGP_MAX_ARCS} arcs; this graph has {graph.num_nodes} / {graph.num_arcs} (posterior_beam gives "
                             "the beam-pruned sum, which takes it)")
        if beam is None and max_active is not None:
            raise ValueError("max_active belongs to the beam search: give a beam (inf for none) with it")
        if nbest is not None and beam is not None:
            raise ValueError("nbest belongs to the dense search: n-best over the token-passing search (beam) is not built")
        assert features.shape[0] == features_length.shape[0]
        logits, lens = self.ctc_logits_windowed(features, features_length, window, margin)
        if beam is None:
            outs = ops.ctc_graph_decode(logits, lens, graph)
        else:
            outs = self._graph_beam_decode(logits, lens, graph, beam, 16384 if max_active is None else int(max_active), int(workspace_cap))
        score, _, _, _, n_trav, arc, start, end, logp = outs[:9]
        B, M = arc.shape
        packed = torch.cat([score.double(), n_trav.double(), arc.double().flatten(), start.double().flatten(), end.double().flatten(),
                            logp.double().flatten()]).cpu()
        sc, n, (a, s, e, lg) = packed[:B], packed[B: 2 * B], packed[2 * B:].split(B * M)
        rate = self.encoder.embed.subsampling_rate
        times = (lambda t0, t1: frame_times(t0, t1, rate, frame_shift_ms)) if with_times else None
        results = graph_results(graph, sc.tolist(), n.tolist(), a.view(B, M).tolist(), s.view(B, M).tolist(), e.view(B, M).tolist(),
                                lg.view(B, M).tolist(), times)
        if posterior or posterior_beam is not None:
            if posterior_beam is None:
                mass = ops.ctc_graph_logp(logits, lens, graph).cpu().tolist()
            else:
                mass = self._graph_beam_logp(logits, lens, graph, float(posterior_beam), 16384 if max_active is None else int(max_active),
                                             int(workspace_cap))[0].cpu().tolist()
            for res, m, best in zip(results, mass, score.cpu().tolist()):
                if res.feasible:
                    res.log_mass, res.posterior = m, min(math.exp(best - m), 1.0)
        if nbest is not None:
            for res, hyps in zip(results, self._graph_nbest_host(logits, lens, graph, int(nbest), distinct, int(workspace_cap))[0]):
                res.nbest = hyps
        return results

    @staticmethod
    def _graph_nbest_host(logits, lens, graph, nbest, distinct, workspace_cap=1 << 30):
        """ops.ctc_graph_nbest and ONE D2H copy of its results -> (per utterance its GraphHypothesis list, the device tensors)."""
        from openeat_amd.utils.decoding_graph import graph_hypotheses
        outs = ops.ctc_graph_nbest(logits, lens, graph, nbest, distinct, workspace_cap=workspace_cap)
        n_hyp, hyp_score, hyp_len, hyp_arcs, hyp_tokens = outs
        B, K, M = hyp_arcs.shape
        packed = torch.cat([n_hyp.double(), hyp_score.double().flatten(), hyp_len.double().flatten(), hyp_arcs.double().flatten(),
                            hyp_tokens.double().flatten()]).cpu()
        n, sc, ln, (ar, tk) = packed[:B], packed[B: B + B * K], packed[B + B * K: B + 2 * B * K], packed[B + 2 * B * K:].split(B * K * M)
        as_int = lambda t, *shape: t.long().view(*shape).tolist()
        return graph_hypotheses(graph, as_int(n, B), sc.view(B, K).tolist(), as_int(ln, B, K), as_int(ar, B, K, M), as_int(tk, B, K, M)), outs

    @torch.no_grad()
    def graph_attention_rescoring(self, features: torch.Tensor, features_length: torch.Tensor, graph, nbest: int = 4,
                                  ctc_weight: float = 0.0, reverse_weight: float = 0.0, lm: Optional[torch.nn.Module] = None,
                                  lm_weight: float = 0.0):
        """The two-pass decode with a grammar as the first pass (WeNet rescores the n-best of its TLG lattice; the reference's
        attention_rescoring takes its n-best from the prefix beam search): ONE encoder pass, the `nbest` best distinct token
        sequences of `graph` on the CTC logits (ops.ctc_graph_nbest, distinct="tokens"; semantics at oe_ctc_graph_nbest), then
        the bi-decoder pass and the score mix of attention_rescoring_batch (asr_model.py:504-528) over all B x nbest
        hypotheses, their graph scores as the CTC scores.  Returns per utterance the picked GraphHypothesis - score the mixed
        score, rank its place in the first pass; for an utterance the graph cannot accept, an infeasible GraphHypothesis (score -inf,
        rank -1, feasible False)."""
        from openeat_amd.utils.decoding_graph import DecodingGraph, GraphHypothesis
        if not isinstance(graph, DecodingGraph):
            raise ValueError(f"graph must be an openeat_amd.utils.decoding_graph.DecodingGraph (got {type(graph).__name__})")
        if reverse_weight > 0 and self.decoder.r_num_blocks == 0:
            raise IndexError("reverse_weight > 0 needs r_decoder_num_blocks > 0 (as in the reference)")
        assert features.shape[0] == features_length.shape[0]
        nbest = int(nbest)
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        lens = encoder_mask.squeeze(1).sum(1)
        hyps, (n_hyp, hyp_score, hyp_len, _, hyp_tokens) = self._graph_nbest_host(self.ctc.logits(encoder_out), lens, graph, nbest, "tokens")
        B, K, M = hyp_tokens.shape
        Lm = max(max((len(h.tokens) for hs in hyps for h in hs), default=0), 1)
        _, _, _, best, mixed = self._rescore_stage2(encoder_out, encoder_mask, hyp_tokens.view(B * K, M), hyp_len.view(B * K),
                                                    hyp_score.view(B * K).double(), Lm, K, ctc_weight, reverse_weight, lm, lm_weight,
                                                    with_scores=True)
        best, mixed = best.cpu().tolist(), mixed.cpu().tolist()
        picks = []
        for b in range(B):
            if not hyps[b]:
                picks.append(GraphHypothesis(rank=-1))
                continue
            h = hyps[b][best[b]]
            h.score = float(mixed[b][best[b]])
            picks.append(h)
        return picks

    @staticmethod
    def _graph_beam_decode(logits, lens, graph, beam, max_active, workspace_cap):
        """ops.ctc_graph_beam_decode with ctc_graph_search's retry: the utterances that overflowed run again with max_active
        doubled, while one utterance's workspace fits workspace_cap.  One D2H copy of status and peak per round."""
        B, T, _ = logits.shape
        outs = ops.ctc_graph_beam_decode(logits, lens, graph, beam, max_active, workspace_cap=workspace_cap)
        while True:
            status, peak = torch.stack([outs[9], outs[10]]).cpu().tolist()
            over = [b for b in range(B) if status[b] == hip.CTC_GRAPH_BEAM_OVERFLOW]
            if not over:
                return outs
            max_active = min(max(2 * max_active, max(peak[b] for b in over)), graph.num_nodes + graph.num_arcs)   # Q + A never overflows
            need = hip.lib().oe_ctc_graph_beam_workspace_bytes(1, T, len(graph.cols), graph.num_nodes, graph.num_arcs, max_active)
            if need > workspace_cap:
                b = max(over, key=lambda i: peak[i])
                raise RuntimeError(f"ctc_graph_search: utterance {b} keeps {peak[b]} states alive in one frame (peak), and max_active="
                                   f"{max_active} needs {need} bytes of workspace for one utterance, over workspace_cap={workspace_cap}: "
                                   "narrow the beam or raise the cap")
            idx = torch.tensor(over, device=logits.device)
            part = ops.ctc_graph_beam_decode(logits[idx], lens[idx], graph, beam, max_active, workspace_cap=workspace_cap)
            for whole, redone in zip(outs, part):
                whole[idx] = redone

    @staticmethod
    def _graph_beam_logp(logits, lens, graph, beam, max_active, workspace_cap):
        """ops.ctc_graph_beam_logp with _graph_beam_decode's retry, differentiable: the utterances that overflowed run again
        with max_active doubled (and at least their peak), while one utterance's gradient workspace fits workspace_cap.  One D2H
        copy of status and peak per round.  -> (logp, status, peak)."""
        B, T, _ = logits.shape
        logp, status, peak = ops.ctc_graph_beam_logp(logits, lens, graph, beam, max_active, workspace_cap=workspace_cap)
        while True:
            st, pk = torch.stack([status, peak]).cpu().tolist()
            over = [b for b in range(B) if st[b] == hip.CTC_GRAPH_BEAM_OVERFLOW]
            if not over:
                return logp, status, peak
            max_active = min(max(2 * max_active, max(pk[b] for b in over)), graph.num_nodes + graph.num_arcs)   # Q + A never overflows
            need = hip.lib().oe_ctc_graph_beam_logp_grad_workspace_bytes(1, T, len(graph.cols), graph.num_nodes, graph.num_arcs, max_active)
            if need > workspace_cap:
                b = max(over, key=lambda i: pk[i])
                raise RuntimeError(f"ctc_graph_beam_logp: utterance {b} keeps {pk[b]} states alive in one frame (peak), and max_active="
                                   f"{max_active} needs {need} bytes of workspace for one utterance, over workspace_cap={workspace_cap}: "
                                   "narrow the beam or raise the cap")
            idx = torch.tensor(over, device=logits.device)
            part = ops.ctc_graph_beam_logp(logits[idx], lens[idx], graph, beam, max_active, workspace_cap=workspace_cap)
            logp = logp.index_copy(0, idx, part[0])
            status, peak = status.index_copy(0, idx, part[1]), peak.index_copy(0, idx, part[2])

    @torch.no_grad()
    def ctc_topk_windowed(self, features: torch.Tensor, features_length: torch.Tensor, beam_size: int, window: Optional[int],
                          margin: int = 16):
        """The per-frame top-`beam_size` CTC log-probabilities of whole recordings, window by window: a generator over
        utils.segment.window_plan that yields, for k = 0, 1, ..., (top_p (B, window, beam) float32, top_i (B, window, beam)
        int64, lens (B) int32): the kept frames of the k-th window of every recording, lens[b] of them (0 for a recording that
        has ended).  Only the k-th windows are encoded, as one batch, and only their kept frames' top-k rows are kept: the
        (T', V) logits of a recording never exist.  window None: one window holds the longest recording."""
        from openeat_amd.utils.segment import encoder_frames, window_plan
        embed = self.encoder.embed
        rate, rc = embed.subsampling_rate, embed.right_context
        n_feats = [int(n) for n in features_length.tolist()]
        n_enc = [encoder_frames(n, rate, rc) for n in n_feats]
        window = max(n_enc + [1]) if window is None else min(int(window), max(n_enc + [1]))
        plans = [window_plan(n, window, margin, rate, rc) for n in n_feats]
        B, dev = len(n_feats), features.device
        for k in range(max(len(p) for p in plans)):
            live = [b for b in range(B) if k < len(plans[b])]
            lg = self._span_logits(features, features_length, [(b, *plans[b][k][:2]) for b in live])
            kept = lg.new_zeros(B, window, lg.shape[2])
            lens = [0] * B
            for w, b in enumerate(live):
                _, _, q0, q1, _ = plans[b][k]
                kept[b, : q1 - q0] = lg[w, q0:q1]
                lens[b] = q1 - q0
            top_p, top_i = ops.topk_rows(kept, beam_size, log_softmax=True)
            yield top_p, top_i, torch.tensor(lens, dtype=torch.int32).to(dev)

    @torch.no_grad()
    def transcribe_long(self, features: torch.Tensor, features_length: torch.Tensor, beam_size: int = 10, window: Optional[int] = 512,
                        margin: int = 16, lm=None, lm_weight: float = 0.0, length_bonus: float = 0.0, context=None,
                        with_times: bool = False, frame_shift_ms: float = 10, on_partial=None, overlap: bool = False):
        """Long-form transcription, the counterpart of ctc_segment (the reference has none; semantics in include/openeat_hip.h,
        oe_ctc_prefix_beam_chunk): ctc_topk_windowed feeds a resumable CTC prefix beam search (utils.stream_search), plain or
        with lm (an NgramLM) and / or context (a ContextGraph) as ctc_lm_beam_search / ctc_context_beam_search take them, so
        neither the logits nor the back-pointers of a whole recording exist.  on_partial(b, tokens, frames) is called whenever
        recording b's stable prefix - the tokens every live prefix shares, final from then on - has grown, with all of it.
        overlap: window k+1 is encoded on a side stream while chunk k is searched.  -> per recording {"tokens", "frames" (the
        encoder frame at which each token entered the beam; with_times "times", the (start_s, end_s) of that frame by
        utils.align.frame_times), "score" (total), "ctc", "lm", "bias"} of the best hypothesis.  Needs the device beam and
        beam_size <= 16 (ValueError otherwise: there is no host implementation)."""
        from openeat_amd.utils.segment import encoder_frames
        from openeat_amd.utils.stream_search import PrefixBeamStream
        # a weight without the part it weighs is dropped: the plain search takes none
        spec = hip.PrefixSearch(beam_size, lm, context, lm_weight if lm is not None else 0.0,
                                length_bonus if (lm is not None or context is not None) else 0.0)
        spec.validate("transcribe_long", DEVICE_BEAM)
        B = features.shape[0]
        assert B == features_length.shape[0]
        embed = self.encoder.embed
        rate = embed.subsampling_rate
        max_len = max(max(encoder_frames(int(n), rate, embed.right_context) for n in features_length.tolist()), 1)
        search = PrefixBeamStream.of(spec, B, max_len, features.device)
        windows = self.ctc_topk_windowed(features, features_length, beam_size, window, margin)
        main = torch.cuda.current_stream(features.device)
        side = torch.cuda.Stream(features.device) if overlap else None

        def fetch():
            """The next window's top-k, or None behind the last; with overlap it is produced on the side stream."""
            if side is None:
                return next(windows, None)
            side.wait_stream(main)                                 # the features, and the buffers the last search has let go of
            with torch.cuda.stream(side):
                got = next(windows, None)
            return got

        seen = [0] * B
        chunk = fetch()
        if chunk is None:
            raise ValueError("transcribe_long: nothing to transcribe")
        while chunk is not None:
            if side is not None:
                main.wait_stream(side)
                for t in chunk:
                    t.record_stream(main)
            ahead = fetch()                                        # with overlap: runs beside the search below
            out = search.push(*chunk, last=ahead is None, emit=False, raw=True)
            if on_partial is not None and ahead is not None:
                n = out["stable_len"].cpu().tolist()               # drains the stream: the price of a partial result
                for b in range(B):
                    if n[b] > seen[b]:
                        seen[b] = n[b]
                        on_partial(b, out["stable_prefix"][b, : n[b]].cpu().tolist(), out["stable_frame"][b, : n[b]].cpu().tolist())
            chunk = ahead
        hip.check_prefix_beam_status(out["status"][0], "transcribe_long")           # the read drains the stream
        n = out["plen"][:, 0].cpu().tolist()
        width = max(n + [1])
        toks, frames = out["prefixes"][:, 0, :width].cpu().numpy(), out["frames"][:, 0, :width].cpu().numpy()
        scores = [out[k][:, 0].cpu().tolist() for k in hip.SCORES]         # (a part the search has not: zeros)
        res = []
        for b in range(B):
            fr = frames[b, : n[b]].tolist()
            if on_partial is not None and n[b] > seen[b]:          # at the end the best hypothesis is all stable
                on_partial(b, toks[b, : n[b]].tolist(), fr)
            r = {"tokens": toks[b, : n[b]].tolist(), "frames": fr, "score": scores[0][b], "ctc": scores[1][b], "lm": scores[2][b],
                 "bias": scores[3][b]}
            if with_times:
                r["times"] = [frame_times(f, f, rate, frame_shift_ms) for f in fr]
            res.append(r)
        return res

    @torch.no_grad()
    def error_counts(self, features: torch.Tensor, features_length: torch.Tensor, targets: torch.Tensor,
                     targets_length: torch.Tensor, mode: str = "ctc_greedy_search", beam_size: int = 10,
                     nbest_oracle: bool = False, **decode_kwargs) -> dict:
        """Decode and score against the targets on the device (ops.edit_distance; the counts of the reference's
        tools/compute-wer.py, semantics in include/openeat_hip.h).  Returns device tensors: `counts` (B, 4) int32 = cor, sub,
        del, ins per utterance, and with nbest_oracle (attention_rescoring on the device beam) `oracle_counts` (B, 4) /
        `oracle_index` (B): the n-best slot with the fewest errors.  Only targets_length is trusted, not the padding.
        ctc_greedy_search reads nothing back; attention_rescoring scores the lists attention_rescoring_batch(**decode_kwargs)
        returns, and nbest_oracle runs the encoder and the prefix beam a second time for the n-best lists (the batched call
        does not hand them out).  The token matrices are as wide as the encoder output; oe_edit_distance takes 1023 columns, so
        of a hypothesis longer than that (more than 41 s of audio decoded to a token per frame) the first 1023 tokens count."""
        from openeat_amd.utils.error_rate import nbest_oracle as oracle_of
        assert features.shape[0] == features_length.shape[0] == targets.shape[0] == targets_length.shape[0]
        device = features.device
        if mode == "ctc_greedy_search":
            if nbest_oracle:
                raise ValueError("error_counts: ctc_greedy_search has no n-best list")
            toks, n = self._ctc_greedy(features, features_length)
            return {"counts": ops.edit_distance(targets, targets_length, toks[:, :EDIT_DISTANCE_MAX], n)}
        if mode != "attention_rescoring":
            raise ValueError(f"error_counts: unknown mode {mode!r}")
        if nbest_oracle and not _device_beam(beam_size):
            raise NotImplementedError("error_counts: nbest_oracle needs the device beam (OE_DEVICE_BEAM=1, beam_size <= 16)")
        hyps = self.attention_rescoring_batch(features, features_length, beam_size, **decode_kwargs)
        hl = [len(h) for h in hyps]
        pad = torch.full((len(hyps), max(hl + [0])), self.ignore_id, dtype=torch.int32)
        for b, h in enumerate(hyps):
            pad[b, : hl[b]] = torch.tensor(h, dtype=torch.int32)
        out = {"counts": ops.edit_distance(targets, targets_length, pad.to(device), torch.tensor(hl, dtype=torch.int32).to(device))}
        if nbest_oracle:
            _, _, pre, plen, _, _, _ = self._rescore_stage1(features, features_length, hip.PrefixSearch(beam_size))
            out["oracle_counts"], out["oracle_index"] = oracle_of(
                ops.edit_distance(targets, targets_length, pre[:, :EDIT_DISTANCE_MAX], plen, group=beam_size), beam_size)
        return out

    def _ctc_prefix_beam_search(self, features, features_length, beam_size: int):
        """asr_model.py:328-396 (batch of one): log-probs and per-frame top-k on the device, the prefix
        recursion in native host code (oe_ctc_prefix_beam_host: same ordering and float64 arithmetic)."""
        assert features.shape[0] == features_length.shape[0]
        assert features.shape[0] == 1
        encoder_out, _, _, top_p, top_i = self._ctc_topk(features, features_length, beam_size)
        if _device_beam(beam_size):                                # (the reference searches every frame of its one utterance)
            return hip.ctc_prefix_beam_device(top_p, top_i, None, beam_size)[0], encoder_out
        return hip.ctc_prefix_beam_host(top_p[0].cpu(), top_i[0].cpu(), beam_size), encoder_out

    def ctc_prefix_beam_search(self, features, features_length, beam_size: int) -> List[int]:
        hyps, _ = self._ctc_prefix_beam_search(features, features_length, beam_size)
        return hyps[0][0]

    @torch.no_grad()
    def ctc_lm_beam_search(self, features, features_length, beam_size: int, lm, lm_weight: float, length_bonus: float = 0.0,
                           eos: bool = True):
        """CTC prefix beam search with n-gram LM shallow fusion, batched (oe_ctc_prefix_beam, lm; semantics in
        include/openeat_hip.h): prefixes are pruned every frame by log_add(pb, pnb) + lm_weight * LM + length_bonus * len.
        -> per utterance [(prefix tuple, total, ctc, lm)] sorted by total.  Needs an NgramLM, the device beam and
        beam_size <= 16 (ValueError otherwise: there is no host implementation)."""
        spec = hip.PrefixSearch(beam_size, lm, None, lm_weight, length_bonus, eos)
        spec.validate("ctc_lm_beam_search", DEVICE_BEAM, require=("lm",))
        return hip._shaped(self._prefix_beam_search("ctc_lm_beam_search", features, features_length, spec), False, "total", "ctc", "lm")

    @torch.no_grad()
    def ctc_context_beam_search(self, features, features_length, beam_size: int, context, lm=None, lm_weight: float = 0.0,
                                length_bonus: float = 0.0, eos: bool = True):
        """CTC prefix beam search with hotword biasing, batched (oe_ctc_prefix_beam, ctx; semantics in include/openeat_hip.h):
        prefixes are pruned every frame by ctc_lm_beam_search's total (the LM term only with an NgramLM) + bias(prefix), the
        score `context`, a ContextGraph, gives the hotwords a prefix holds, plus a per-token credit while one is half spoken;
        at the end of the utterance the pending credit is dropped.  -> per utterance [(prefix tuple, total, ctc, lm, bias)]
        sorted by total.  Needs the device beam and beam_size <= 16 (ValueError otherwise: there is no host implementation)."""
        spec = hip.PrefixSearch(beam_size, lm, context, lm_weight, length_bonus, eos)
        spec.validate("ctc_context_beam_search", DEVICE_BEAM, require=("context",))
        return hip._shaped(self._prefix_beam_search("ctc_context_beam_search", features, features_length, spec), False, *hip.SCORES)

    def _prefix_beam_search(self, caller, features, features_length, spec):
        """_ctc_topk and on it the device prefix search `spec`, a hip.PrefixSearch -> the hip.PrefixBeamResult, status checked."""
        assert features.shape[0] == features_length.shape[0]
        _, _, lens, top_p, top_i = self._ctc_topk(features, features_length, spec.beam)
        return hip._prefix_beam_device(caller, top_p, top_i, lens, spec, False)

    def attention_rescoring(self, features, features_length, beam_size: int, ctc_weight: float = 0.0,
                            reverse_weight: float = 0.0, lm: Optional[torch.nn.Module] = None, lm_weight: float = 0,
                            autoregressive: bool = True, token2char: dict = {}):
        """asr_model.py:418-534."""
        assert features.shape[0] == features_length.shape[0] == 1
        device = features.device
        hyps, encoder_out = self._ctc_prefix_beam_search(features, features_length, beam_size)
        assert len(hyps) == beam_size
        lens = torch.tensor([len(h[0]) for h in hyps], device=device, dtype=torch.long)
        Lm = int(lens.max())
        ori = torch.full((beam_size, Lm), self.ignore_id, dtype=torch.long, device=device)
        for i, h in enumerate(hyps):
            ori[i, : len(h[0])] = torch.tensor(h[0], dtype=torch.long, device=device)
        hyps_pad, _ = add_sos_eos(ori, self.sos, self.eos, self.ignore_id)
        in_lens = lens + 1
        L = hyps_pad.size(1)
        hyps_mask = (~make_pad_mask(in_lens, L)).unsqueeze(1) & subsequent_mask(L, device=device).unsqueeze(0)
        enc = encoder_out.repeat(beam_size, 1, 1)
        enc_mask = torch.ones(beam_size, 1, enc.size(1), dtype=torch.bool, device=device)
        r_pad = reverse_pad_list(ori, lens, self.ignore_id)
        r_hyps_pad, _ = add_sos_eos(r_pad, self.sos, self.eos, self.ignore_id)
        if reverse_weight > 0 and self.decoder.r_num_blocks == 0:
            raise IndexError("reverse_weight > 0 needs r_decoder_num_blocks > 0 (as in the reference)")
        decoder_out, r_decoder_out, pre = self.decoder(enc, enc_mask, hyps_pad, r_hyps_pad, hyps_mask)
        l_lp = ops.log_softmax_rows(decoder_out).cpu().numpy()
        r_lp = ops.log_softmax_rows(r_decoder_out).cpu().numpy() if self.decoder.r_num_blocks > 0 else None
        use_nn_lm = lm_weight > 0 and isinstance(lm, torch.nn.Module)
        lm_lp = None
        if use_nn_lm:
            # asr_model.py:490-499 (the reference calls `lm.encoder(tokens, lengths)`, meaning the LM's forward up to the
            # projection; see openeat_amd/models/language_model.py).  Autoregressive LM: scored on sos + hypothesis.
            if autoregressive:
                lm_lp = lm.log_probs(hyps_pad, in_lens).cpu().numpy()
            else:
                lm_in = ori.masked_fill(ori == self.ignore_id, self.eos)
                lm_lp = lm.log_probs(lm_in, in_lens - 1).cpu().numpy()
        best, best_i = -float("inf"), 0
        for i, (hyp, ctc_score) in enumerate(hyps):
            score = sum(l_lp[i][j][w] for j, w in enumerate(hyp)) + l_lp[i][len(hyp)][self.eos]
            lm_score = 0.0
            if use_nn_lm:
                lm_score = sum(lm_lp[i][j][w] for j, w in enumerate(hyp))
            elif lm_weight > 0 and lm is not None:
                lm_score = lm.score(" ".join(token2char[w] for w in hyp), bos=True, eos=True)
            if reverse_weight > 0:
                r = sum(r_lp[i][len(hyp) - j - 1][w] for j, w in enumerate(hyp)) + r_lp[i][len(hyp)][self.eos]
                score = score * (1 - reverse_weight) + r * reverse_weight
            score += ctc_score * ctc_weight + lm_score * lm_weight
            if score > best:
                best, best_i = score, i
        return hyps[best_i][0], enc, pre

    @torch.no_grad()
    def attention_rescoring_batch(self, features: torch.Tensor, features_length: torch.Tensor, beam_size: int,
                                  ctc_weight: float = 0.0, reverse_weight: float = 0.0,
                                  lm: Optional[torch.nn.Module] = None, lm_weight: float = 0.0,
                                  use_graphs: Optional[bool] = None, first_pass_lm: bool = False,
                                  first_pass_lm_weight: Optional[float] = None, length_bonus: float = 0.0,
                                  context=None) -> List[List[int]]:
        """Batched form of attention_rescoring (the reference handles one utterance per call,
        asr_model.py:444): ONE encoder pass and ONE fused log-softmax top-k for the whole batch, the prefix
        recursion of every utterance on its own valid frames (one wave each on the device; OE_DEVICE_BEAM=0: native host
        code), then ONE bi-decoder pass over all B x beam hypotheses and the same score mix (asr_model.py:504-528).
        use_graphs (default: OE_DECODE_GRAPHS, off): replay the two stages from HIP graphs cached per shape.
        first_pass_lm: with an NgramLM and lm_weight > 0 the n-best lists come from the LM-fused search (ctc_lm_beam_search's
        kernel, pruning by CTC + first_pass_lm_weight * LM + length_bonus * length; the weight defaults to lm_weight); the
        rescoring itself is unchanged and takes the prefixes' plain CTC scores.
        context: a ContextGraph of hotwords - the n-best lists come from the biased search (ctc_context_beam_search's kernel,
        with the LM only under the first_pass_lm rule, and with length_bonus), and every hypothesis' final bias is added to
        its mixed score, since nothing else in the rescoring knows about hotwords.  Device beam only."""
        device = features.device
        B = features.shape[0]
        R = B * beam_size
        if reverse_weight > 0 and self.decoder.r_num_blocks == 0:
            raise IndexError("reverse_weight > 0 needs r_decoder_num_blocks > 0 (as in the reference)")
        graphs = DECODE_GRAPHS if use_graphs is None else bool(use_graphs)
        spec = hip.PrefixSearch.first_pass(beam_size, lm, lm_weight, first_pass_lm, first_pass_lm_weight, length_bonus, context)
        if not spec.plain:                                         # (the plain search alone has a host implementation)
            spec.validate("attention_rescoring_batch", DEVICE_BEAM)
        on_device = _device_beam(beam_size)
        if on_device and graphs:
            return self._rescoring_batch_graphs(features, features_length, spec, ctc_weight, reverse_weight, lm, lm_weight)
        if on_device:
            encoder_out, encoder_mask, pre, plen, ctc_scores, bad, bias = self._rescore_stage1(features, features_length, spec)
            Lm = max(int(plen.max()), 1)                           # the one host sync of the n-best stage
            hip.check_prefix_beam_status(bad)
            toks, n, mean_len = self._rescore_stage2(encoder_out, encoder_mask, pre, plen, ctc_scores, Lm, beam_size, ctc_weight,
                                                     reverse_weight, lm, lm_weight, bias)
            self.last_nbest_mean_len = float(mean_len)
            toks, n = toks.cpu(), n.cpu().tolist()
            return [toks[b, : n[b]].tolist() for b in range(B)]
        encoder_out, encoder_mask, lens, top_p, top_i = self._ctc_topk(features, features_length, beam_size)
        nbest = hip.ctc_prefix_beam_host_batch(top_p.cpu(), top_i.cpu(), lens.cpu().tolist(), beam_size)
        for b in range(B):                                         # a very short utterance can yield fewer than `beam` prefixes
            while len(nbest[b]) < beam_size:
                nbest[b].append((nbest[b][-1][0], -float("inf")))
        flat = [h for nb in nbest for h in nb]
        self.last_nbest_mean_len = sum(len(h[0]) for h in flat) / max(len(flat), 1)
        hl = torch.tensor([len(h[0]) for h in flat], dtype=torch.long)
        Lm = max(int(hl.max()), 1)
        ori = torch.full((R, Lm), self.ignore_id, dtype=torch.long)
        for i, h in enumerate(flat):
            if h[0]:
                ori[i, : len(h[0])] = torch.tensor(h[0], dtype=torch.long)
        ctc_scores = torch.tensor([h[1] for h in flat], dtype=torch.float64, device=device)
        best = self._rescore_scores(encoder_out, encoder_mask, ori.to(device), hl.to(device), ctc_scores, torch.isinf(ctc_scores), Lm,
                                    beam_size, ctc_weight, reverse_weight, lm, lm_weight).cpu().tolist()
        return [list(nbest[b][best[b]][0]) for b in range(B)]

    # ---- the pieces of the batched rescoring (each of fixed shape given (B, T) resp. (B, T', L): capturable) --------------
    def _rescore_stage1(self, features, features_length, spec):
        """Encoder, CTC projection, fused log-softmax top-k and the prefix recursion `spec` (a hip.PrefixSearch) - all on the
        device, no host sync.  Returns encoder_out, encoder_mask, prefixes (R, T') int32, lengths (R) int32 (-1: the slot does
        not exist), CTC scores (R) float64, status word, the hypotheses' final bias (R) float64 (None without a graph)."""
        encoder_out, encoder_mask, lens, top_p, top_i = self._ctc_topk(features, features_length, spec.beam)
        r = hip._prefix_beam_device("attention_rescoring_batch", top_p, top_i, lens, spec, True)
        R = r.plen.numel()
        return (encoder_out, encoder_mask, r.prefixes.view(R, -1), r.plen.view(R), r.ctc.view(R), r.status,
                None if r.bias is None else r.bias.view(R))

    def _rescore_stage2(self, encoder_out, encoder_mask, pre, plen, ctc_scores, Lm, beam_size, ctc_weight, reverse_weight, lm, lm_weight,
                        bias=None, with_scores=False):
        """The n-best lists as device tensors -> (tokens (B, Lm) of the rescored pick, their lengths (B), mean n-best length).
        Lm >= the longest hypothesis (any padding is ignore_id and masked).  bias (R) float64: added to the mixed scores.
        with_scores: also the pick's slot (B) and the mixed scores (B, beam) float64 it is the arg-max of."""
        device = pre.device
        B = encoder_out.shape[0]
        missing = plen < 0
        hl = plen.clamp(min=0).long()
        ori = pre[:, :Lm].long()
        ori = ori.masked_fill(torch.arange(Lm, device=device).unsqueeze(0) >= hl.unsqueeze(1), self.ignore_id)
        ctc_scores = ctc_scores.masked_fill(missing, -float("inf"))
        if with_scores:
            mixed = self._rescore_mix(encoder_out, encoder_mask, ori, hl, ctc_scores, missing, Lm, beam_size, ctc_weight, reverse_weight,
                                      lm, lm_weight, bias)
            best = mixed.argmax(1)
            pick = best + torch.arange(B, device=device) * beam_size
            return ori.index_select(0, pick), hl.index_select(0, pick), hl.float().mean(), best, mixed
        best = self._rescore_scores(encoder_out, encoder_mask, ori, hl, ctc_scores, missing, Lm, beam_size, ctc_weight, reverse_weight,
                                    lm, lm_weight, bias)
        pick = best + torch.arange(B, device=device) * beam_size
        return ori.index_select(0, pick), hl.index_select(0, pick), hl.float().mean()

    def _rescore_scores(self, encoder_out, encoder_mask, ori, hl, ctc_scores, missing, Lm, beam_size, ctc_weight, reverse_weight, lm,
                        lm_weight, bias=None):
        """asr_model.py:504-528 for all B x beam hypotheses at once: index of the best hypothesis per utterance.
        bias (R) float64 or None: the hypotheses' hotword scores, added to the mix."""
        return self._rescore_mix(encoder_out, encoder_mask, ori, hl, ctc_scores, missing, Lm, beam_size, ctc_weight, reverse_weight, lm,
                                 lm_weight, bias).argmax(1)

    def _rescore_mix(self, encoder_out, encoder_mask, ori, hl, ctc_scores, missing, Lm, beam_size, ctc_weight, reverse_weight, lm,
                     lm_weight, bias=None):
        """_rescore_scores before the arg-max: the mixed scores (B, beam) float64, -inf for a missing slot."""
        device = ori.device
        B = encoder_out.shape[0]
        R = B * beam_size
        hyps_pad, _ = add_sos_eos(ori, self.sos, self.eos, self.ignore_id)
        L = hyps_pad.size(1)
        hyps_mask = (~make_pad_mask(hl + 1, L)).unsqueeze(1) & subsequent_mask(L, device=device).unsqueeze(0)
        enc = encoder_out.repeat_interleave(beam_size, dim=0)
        enc_mask = encoder_mask.repeat_interleave(beam_size, dim=0)
        r_ori = reverse_pad_list(ori, hl, self.ignore_id)
        r_hyps_pad, _ = add_sos_eos(r_ori, self.sos, self.eos, self.ignore_id)
        with ops.causal_self_attention():                                        # hyps_mask is causal: key blocks above the diagonal are skipped
            l_x, r_x, _ = self.decoder(enc, enc_mask, hyps_pad, r_hyps_pad, hyps_mask)
        pos = torch.arange(L, device=device).unsqueeze(0)
        valid = pos < hl.unsqueeze(1)                                            # token positions j < len
        tok = torch.cat([ori, ori.new_full((R, L - Lm), self.ignore_id)], 1).clamp(min=0)

        def seq_score(logits, tokens_at):
            # the token's and <eos>'s log-probability at every position, straight from the logits (no (R, L, V) log-softmax)
            tok_lp, eos_all = ops.logprob_gather(logits, tokens_at, also=self.eos)
            eos_lp = eos_all.gather(1, hl.unsqueeze(1)).squeeze(1)
            return (tok_lp * valid).sum(1).double() + eos_lp.double()

        score = seq_score(l_x, tok)
        if reverse_weight > 0:
            r_tok = torch.cat([r_ori.long(), ori.new_full((R, L - Lm), self.ignore_id)], 1).clamp(min=0)
            score = score * (1 - reverse_weight) + seq_score(r_x, r_tok) * reverse_weight
        score = score + ctc_scores * ctc_weight
        if isinstance(lm, NgramLM) and lm_weight > 0:                             # n-gram LM (asr_model.py:515-516, 528): log10, as kenlm's
            score = score + ops.ngram_score(lm, ori, hl) * lm_weight
        elif lm is not None and lm_weight > 0:                                    # neural-LM shallow fusion (asr_model.py:490-527)
            lm_tok = ops.logprob_gather(lm.logits(hyps_pad, hl + 1), tok) if hasattr(lm, "logits") else \
                lm.log_probs(hyps_pad, hl + 1).gather(2, tok.unsqueeze(2)).squeeze(2)
            score = score + (lm_tok * valid).sum(1).double() * lm_weight
        if bias is not None:
            score = score + bias
        score = score.masked_fill(missing, -float("inf"))         # (0 * -inf above would be nan: the slot is out whatever the weights)
        return score.view(B, beam_size)

    def _rescoring_batch_graphs(self, features, features_length, spec, ctc_weight, reverse_weight, lm, lm_weight):
        """The same two stages replayed from HIP graphs (decode is launch-bound: ~1500 small launches for 64 utterances):
        stage 1 keyed by the feature shape and the search, stage 2 by the n-best length rounded up to a multiple of 16; between
        them the one host read of the longest hypothesis.  A shape is run eagerly the first time it is seen and captured for the
        next; a stage that cannot be captured keeps running eagerly.  At most DECODE_GRAPH_SLOTS graphs per stage are kept.
        The keys hold the LM and the context graph themselves (by identity): the tables a capture points at live as long as it."""
        from openeat_amd.utils import common
        B, beam_size = features.shape[0], spec.beam
        cache = self.__dict__.setdefault("_decode_graphs", {})
        static_before = common.STATIC_SHAPES
        common.STATIC_SHAPES = True                                # label bookkeeping of fixed width: nothing reads a length on the host
        try:
            k1 = ("s1", tuple(features.shape), spec)
            encoder_out, encoder_mask, pre, plen, ctc_scores, bad, bias = _graph_call(
                cache, k1, lambda f, fl: self._rescore_stage1(f, fl, spec), (features, features_length))
            Lm = max(int(plen.max()), 1)
            hip.check_prefix_beam_status(bad)
            Lb = min(-(-Lm // 16) * 16, pre.shape[1])
            k2 = ("s2", tuple(encoder_out.shape), beam_size, Lb, float(ctc_weight), float(reverse_weight), lm, float(lm_weight),
                  bias is not None)                                # (a bias is one more input: a graph of its own)
            toks, n, mean_len = _graph_call(
                cache, k2, lambda *a: self._rescore_stage2(*a[:5], Lb, beam_size, ctc_weight, reverse_weight, lm, lm_weight, a[5]),
                (encoder_out, encoder_mask, pre, plen, ctc_scores, bias))
        finally:
            common.STATIC_SHAPES = static_before
        self.last_nbest_mean_len = float(mean_len)
        toks, n = toks.cpu(), n.cpu().tolist()
        return [toks[b, : n[b]].tolist() for b in range(B)]

    def recognize(self, features: torch.Tensor, features_length: torch.Tensor, beam_size: int = 10) -> torch.Tensor:
        """asr_model.py:205-295: batched attention beam search (incl. the reference's un-reordered cache)."""
        assert features.shape[0] == features_length.shape[0]
        device = features.device
        B = features.shape[0]
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        maxlen, d = encoder_out.size(1), encoder_out.size(2)
        R = B * beam_size
        encoder_out = encoder_out.unsqueeze(1).repeat(1, beam_size, 1, 1).view(R, maxlen, d)
        encoder_mask = encoder_mask.unsqueeze(1).repeat(1, beam_size, 1, 1).view(R, 1, maxlen)
        hyps = torch.full((R, 1), self.sos, dtype=torch.long, device=device)
        scores = torch.tensor([0.0] + [-float("inf")] * (beam_size - 1), device=device).repeat(B).unsqueeze(1)
        end_flag = torch.zeros_like(scores, dtype=torch.bool)
        cache = None
        for i in range(1, maxlen + 1):
            if end_flag.sum() == R:
                break
            hyps_mask = subsequent_mask(i, device=device).unsqueeze(0).repeat(R, 1, 1)
            p, cache, _ = self.decoder.forward_one_step(hyps, hyps_mask, encoder_out, encoder_mask, cache=cache)
            top_k_logp, top_k_index = ops.topk_rows(p, beam_size, log_softmax=True)
            top_k_logp = mask_finished_scores(top_k_logp, end_flag)
            top_k_index = mask_finished_preds(top_k_index, end_flag, self.eos)
            scores = (scores + top_k_logp).view(B, beam_size * beam_size)
            scores, offset_k_index = ops.topk_rows(scores, beam_size)
            scores = scores.view(-1, 1)
            base = torch.arange(B, device=device).view(-1, 1).repeat(1, beam_size) * beam_size * beam_size
            best_k_index = base.view(-1) + offset_k_index.view(-1)
            best_k_pred = torch.index_select(top_k_index.view(-1), dim=-1, index=best_k_index)
            best_hyps_index = best_k_index // beam_size
            hyps = torch.cat((torch.index_select(hyps, 0, best_hyps_index), best_k_pred.view(-1, 1)), dim=1)
            end_flag = torch.eq(hyps[:, -1], self.eos).view(-1, 1)
        scores = scores.view(B, beam_size)
        best_index = torch.argmax(scores, dim=-1).long() + torch.arange(B, dtype=torch.long, device=device) * beam_size
        return torch.index_select(hyps, 0, best_index)[:, 1:]

    @torch.no_grad()
    def ctc_attention_beam_search(self, features: torch.Tensor, features_length: torch.Tensor, beam_size: int = 10,
                                  ctc_weight: float = 0.3, length_bonus: float = 0.0, ctc_candidates: Optional[int] = None,
                                  max_len: Optional[int] = None, nbest: bool = False, lm=None, lm_weight: float = 0.0,
                                  lm_prebeam: bool = True, context=None, context_prebeam: bool = True):
        """Joint CTC/attention one-pass beam search (not in the reference; semantics in utils/joint_search.py and, for the CTC
        prefix score, include/openeat_hip.h): the decoder proposes `ctc_candidates` tokens per hypothesis (default
        min(2 beam_size, V, 64)), and each is ranked by (1 - ctc_weight) * attention + ctc_weight * CTC prefix score +
        length_bonus * length.  One encoder pass and one log-softmax of the CTC logits for the batch, then per step one
        decoder.forward_one_step over all B x beam hypotheses and one oe_ctc_prefix_score launch (none with ctc_weight == 0).
        Unlike recognize, which reproduces the reference's un-reordered decoder cache on purpose, this search reorders the
        per-layer decoder cache by the surviving parents after every pruning.  max_len: the step limit (default: the batch's
        encoder length, as in recognize).  -> per utterance the best hypothesis' tokens without <eos>; nbest: per utterance
        [(tokens, total, att, ctc)], finished hypotheses first, each group by total (ctc is 0 with ctc_weight == 0).
        lm (an NgramLM over this model's vocab_size tokens), lm_weight, lm_prebeam: n-gram LM fusion inside the search - the
        total gains lm_weight * the hypothesis' LM score (log10, </s> included once it is finished), one oe_ngram_next launch
        per step; lm_prebeam: the LM also takes part in choosing the candidates (utils/joint_search.py).  With an LM the
        nbest entries are (tokens, total, att, ctc, lm).
        context (a ContextGraph of hotword phrases over this model's tokens), context_prebeam: hotword biasing inside the
        search - the total gains the hypothesis' bias (hits + the pending partial credit, which <eos> drops;
        include/openeat_hip.h), one oe_context_next launch per step; context_prebeam: the bias also takes part in choosing the
        candidates, at the price of one more launch over the whole vocabulary (utils/joint_search.py).  A phrase with a
        token id >= vocab_size or with <eos> could never fire and is refused.  With a graph the nbest entries gain a last
        element, bias: (tokens, total, att, ctc[, lm], bias)."""
        from openeat_amd.utils.context_graph import ContextGraph
        from openeat_amd.utils.joint_search import joint_beam_search
        if not 0.0 <= ctc_weight <= 1.0:
            raise ValueError(f"ctc_weight must lie in [0, 1] (got {ctc_weight})")
        if self.ctc_weight == 1.0:
            raise ValueError("this model was built with ctc_weight == 1.0: its decoder was never trained")
        C = min(2 * beam_size, self.vocab_size, 64) if ctc_candidates is None else int(ctc_candidates)
        if not 1 <= C <= min(64, self.vocab_size):
            raise ValueError(f"ctc_candidates must lie in 1..{min(64, self.vocab_size)} (got {C})")
        if beam_size < 1:
            raise ValueError(f"beam_size must be >= 1 (got {beam_size})")
        if lm is not None:
            if not isinstance(lm, NgramLM):
                raise ValueError(f"lm must be an NgramLM (got {type(lm).__name__})")
            if not math.isfinite(lm_weight):
                raise ValueError(f"lm_weight must be finite (got {lm_weight})")
            if len(lm.tok2word) != self.vocab_size:
                raise ValueError(f"the LM maps {len(lm.tok2word)} tokens, the model has {self.vocab_size}")
        if context is not None:
            if not isinstance(context, ContextGraph):
                raise ValueError(f"context must be a ContextGraph (got {type(context).__name__})")
            for q in context.phrases:
                if any(t >= self.vocab_size or t == self.eos for t in q):
                    raise ValueError(f"hotword phrase {list(q)} holds <eos> ({self.eos}) or a token id >= vocab_size ({self.vocab_size}): "
                                     "it can never fire")
        assert features.shape[0] == features_length.shape[0]
        device = features.device
        encoder_out, encoder_mask, _ = self._encode(features, features_length)
        lens = encoder_mask.squeeze(1).sum(1).to(torch.int32)
        logp = ops.log_softmax_rows(self.ctc.logits(encoder_out))
        R = features.shape[0] * beam_size
        memory = encoder_out.repeat_interleave(beam_size, dim=0)
        memory_mask = encoder_mask.repeat_interleave(beam_size, dim=0)
        sos = torch.full((R, 1), self.sos, dtype=torch.long, device=device)
        cache = None

        def step_fn(tokens, parents):
            nonlocal cache
            hyps = torch.cat((sos, tokens), dim=1)
            if parents is not None:                                # the survivors' own histories, not their slots'
                cache = [c.index_select(0, parents) for c in cache]
            hyps_mask = subsequent_mask(hyps.size(1), device=device).unsqueeze(0).repeat(R, 1, 1)
            p, cache, _ = self.decoder.forward_one_step(hyps, hyps_mask, memory, memory_mask, cache=cache)
            return ops.log_softmax_rows(p)

        kw = {} if context is None else dict(context=context, context_prebeam=context_prebeam)
        if lm is None:
            res = joint_beam_search(logp, lens, step_fn, beam_size, C, self.eos, ctc_weight, length_bonus, max_len, **kw)
        else:
            res = joint_beam_search(logp, lens, step_fn, beam_size, C, self.eos, ctc_weight, length_bonus, max_len, 0, lm,
                                    float(lm_weight), lm_prebeam, **kw)
        if nbest:
            return [[h[:4] + h[5:] for h in nb] for nb in res]
        return [nb[0][0] if nb else [] for nb in res]
