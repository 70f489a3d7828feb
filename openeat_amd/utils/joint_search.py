"""Joint CTC/attention one-pass beam search (Watanabe et al. 2017, Hori et al. 2017): the attention decoder proposes tokens,
and the CTC prefix score of every proposal (oe_ctc_prefix_score, semantics in include/openeat_hip.h) is mixed into the pruning
key, so that CTC vetoes the decoder's deletions, loops and early <eos> while the decoder supplies the label dependence CTC
lacks.  The reference has no such mode; the yardstick is tests/ctc_prefix_score_ref.py.

The search, per utterance, with `beam`, C candidates per hypothesis, lam = ctc_weight in [0, 1], beta = length_bonus and a
step limit.  A hypothesis carries its tokens g, a = the sum of its attention log-probabilities, k = psi(g) (0 for the empty
one), a finished flag and a total.  It starts from the one empty hypothesis.  At each step an unfinished hypothesis yields C
candidates, the top-C tokens of its attention log-probabilities l(. | g) in oe_topk_rows order (descending, ties to the
lowest id); candidate c has a' = a + l(c), k' = psi(g . c) and total (1 - lam) a' + lam k' + beta len, len the number of
non-<eos> tokens.  With lam == 0 the CTC term is left out entirely (no 0 * -inf, and no prefix-score launch; k stays 0).
A candidate whose total is -inf is dropped.  A finished hypothesis (last token <eos>) yields itself once, unchanged, in its
slot's position.  The utterance's candidates, in (slot, candidate rank) order, are stably sorted descending by total and the
first `beam` survive.  The search stops when every survivor is finished or the step limit is reached.  Finished hypotheses
come first in the result, in total order, then the unfinished ones.

The attention scores come from a step function, so the loop runs with any scorer: step_fn(tokens, parents) -> (R, V) float32
log-probabilities, where tokens (R, n) int64 are the R = B * beam hypotheses without <sos> (n = 0 at the first step; behind a
finished hypothesis' <eos> the columns repeat <eos>) and parents (R) int64 names, for each row, the row of the previous step
it extends (None at the first step) - what a scorer with a per-row cache reorders its cache by.

The bookkeeping is torch tensor plumbing of fixed shape; one step (score + prune) reads nothing on the host and is capturable.
The totals are float64, which oe_topk_rows (float32) does not take: the prune is a stable descending torch.sort, the same
(slot, rank) tie order.  The loop reads one flag per step on the host, the all-finished test, as ASRModel.recognize does.

With an n-gram LM (`lm`, an openeat_amd.models.ngram_lm.NgramLM, and `lm_weight`; Hori et al. 2017's three-way sum) a hypothesis
also carries m, the float64 left-to-right sum of its tokens' LM terms log10 p(token | <s> + the tokens before it) - for <eos>
the </s> term, so m includes it once the hypothesis is finished.  The terms are oe_ngram_next's (include/openeat_hip.h), in
log10 units, mixed in unconverted as in the fused prefix beam and in the rescoring.  Candidate c has m' = m + term(c) and
    total = (((1 - lam) a' + lam k') + beta len) + lm_weight m',
products and sums each rounded on their own, in this order (with lam == 0 the CTC term is left out, as above); a finished
hypothesis carries m unchanged, as it does a and k.  Which C tokens are candidates depends on `lm_prebeam`:
  True:  one full-vocabulary oe_ngram_next per step gives L (R, V), and the candidates are the top-C tokens, in oe_topk_rows
         order, of the float32 key (l(. | g) in float64 + lm_weight * L) - the LM takes part in the pre-selection; the decoder
         weight deliberately does not enter this key, so with lm_weight == 0 it is l(. | g) to the bit for every ctc_weight,
         1.0 included.  l(c) and term(c) are then gathered from l and L: the exact values, not the key's.
  False: the candidates are the decoder's own top-C, exactly as without an LM, and one candidate-form oe_ngram_next scores
         just those.
With an LM and lm_weight == 0 the n-best lists, their order and the bits of total, att and ctc are those of the search without
an LM, in both modes.  The step stays free of host reads and capturable.  With lm None nothing changes: no code path, no bit,
no launch.  The result rows gain a sixth element, m.

With hotwords (`context`, an openeat_amd.utils.context_graph.ContextGraph) a hypothesis also carries its automaton state, its
hits(g) and its bias(g) as include/openeat_hip.h defines them for the biased prefix search (the empty hypothesis: the root,
hits 0, bias 0).  Candidate c of hypothesis g has (s', h', b') from oe_context_next - b' = bias(g . c) with the pending
partial credit, for <eos> hits(g) alone: the hypothesis ends, the credit is dropped - and
    total = ((((1 - lam) a' + lam k') + beta len) [+ lm_weight m']) + b',
products and sums each rounded on their own, in this order; the LM summand only with an LM, the CTC term left out with
lam == 0, as above.  A finished hypothesis carries state, hits and bias unchanged, as it does a, k and m.  The float32 key
whose top-C, in oe_topk_rows order, are the candidates is
    float32( l(. | g) in float64 [+ lm_weight * L, with an LM and lm_prebeam] [+ (b'(.) - bias(g)), with context_prebeam] ),
the summands in this order, the difference taken in float64 - a difference, because a large standing bias would otherwise eat
the decoder's float32 bits.  With `context_prebeam` one full-vocabulary oe_context_next (out_bias only) feeds the key and one
candidate-form call on the chosen C gives (s', h', b'); without it the candidates are chosen as without a graph and one
candidate-form call scores them.  With no summand beyond l the key is att_logp itself.
The result rows gain a last element, bias: (tokens, total, att, ctc, finished[, lm], bias), the value that entered total - so a
hypothesis that is unfinished at the step limit keeps its pending credit.  With an empty graph, or one whose scores and c are
all zero, the n-best lists, their order and the bits of total, att, ctc and lm are those of the search without `context`, in
both pre-selection modes and with or without an LM.  The step stays free of host reads and capturable.  With context None
nothing changes: no code path, no bit, no launch."""
import math
from typing import Callable, List, NamedTuple, Optional

import torch

from openeat_amd import ops


class BeamState(NamedTuple):
    tokens: torch.Tensor      # (R, n) int64
    parents: Optional[torch.Tensor]   # (R) int64 rows of the previous step, None before the first
    att: torch.Tensor         # (R) float64
    ctc: torch.Tensor         # (R) float64
    total: torch.Tensor       # (R) float64, -inf: the slot does not exist
    finished: torch.Tensor    # (R) bool
    length: torch.Tensor      # (R) int64 non-<eos> tokens
    state: Optional[torch.Tensor]     # (R, Tmax, 2) float64 CTC prefix states (None with ctc_weight == 0)
    lm: Optional[torch.Tensor] = None  # (R) float64 sum of the LM terms (None without an LM)
    cstate: Optional[torch.Tensor] = None  # (R) int32 state in the context graph's automaton (these three: None without a graph)
    hits: Optional[torch.Tensor] = None    # (R) float64 hits(g)
    bias: Optional[torch.Tensor] = None    # (R) float64 bias(g) as it entered total


def _check_lm(lm, lm_weight):
    from openeat_amd.models.ngram_lm import NgramLM
    if not isinstance(lm, NgramLM):
        raise ValueError(f"lm must be an openeat_amd.models.ngram_lm.NgramLM (got {type(lm).__name__})")
    if not math.isfinite(lm_weight):
        raise ValueError(f"lm_weight must be finite (got {lm_weight})")


def _check_context(context):
    from openeat_amd.utils.context_graph import ContextGraph
    if not isinstance(context, ContextGraph):
        raise ValueError(f"context must be an openeat_amd.utils.context_graph.ContextGraph (got {type(context).__name__})")


def initial_state(logp: torch.Tensor, lens: Optional[torch.Tensor], beam: int, ctc_weight: float, blank: int = 0, lm=None,
                  context=None, context_prebeam: bool = True) -> BeamState:
    """The one empty hypothesis per utterance in slot 0; the other slots do not exist yet.  lm / context: the search's LM and
    context graph or None (context_prebeam is the search's, for symmetry: the state does not depend on it)."""
    B, dev = logp.shape[0], logp.device
    R = B * beam
    total = torch.full((B, beam), -float("inf"), dtype=torch.float64, device=dev)
    total[:, 0] = 0.0
    zeros = torch.zeros(R, dtype=torch.float64, device=dev)
    state = ops.ctc_prefix_score_init(logp, lens, group=beam, blank=blank) if ctc_weight > 0 else None
    return BeamState(torch.zeros(R, 0, dtype=torch.int64, device=dev), None, zeros, zeros.clone(), total.view(R),
                     torch.zeros(R, dtype=torch.bool, device=dev), torch.zeros(R, dtype=torch.int64, device=dev), state,
                     None if lm is None else zeros.clone(),
                     *((None, None, None) if context is None else
                       (torch.zeros(R, dtype=torch.int32, device=dev), zeros.clone(), zeros.clone())))


def search_step(logp: torch.Tensor, lens: Optional[torch.Tensor], st: BeamState, att_logp: torch.Tensor, beam: int, C: int, eos: int,
                ctc_weight: float, length_bonus: float, blank: int = 0, cand_state: Optional[torch.Tensor] = None, lm=None,
                lm_weight: float = 0.0, lm_prebeam: bool = True, context=None, context_prebeam: bool = True) -> BeamState:
    """One step: candidates, their CTC prefix scores (and LM terms, with `lm`, and hotword biases, with `context`: st from
    initial_state(..., lm=lm, context=context)), the prune.  att_logp (R, V) float32 for st's rows.  No host read."""
    dev = logp.device
    R = st.total.shape[0]
    B = R // beam
    lam, beta = float(ctc_weight), float(length_bonus)
    ninf = -float("inf")
    alive = st.total > ninf
    live = alive & ~st.finished
    pre_bias = L = None                                                     # what the pre-selection key adds to l(. | g)
    if context is not None:
        _check_context(context)
        if context_prebeam:
            # every row sits in a state of the graph (finished and missing rows too): their entries are finite and masked below
            pre_bias = ops.context_next(context, st.cstate, st.hits, None, eos, V=att_logp.shape[1], want_state=False) - st.bias.unsqueeze(1)
    if lm is not None:
        _check_lm(lm, lm_weight)
        lmw = float(lm_weight)
        # every row is scored on all its columns: the terms of finished and missing rows are finite and masked below
        lm_len = torch.full((R,), st.tokens.shape[1], dtype=torch.int32, device=dev)
        if lm_prebeam:
            if lm.tok2word.shape[0] != att_logp.shape[1]:
                raise ValueError(f"the LM maps {lm.tok2word.shape[0]} tokens, the scorer gives {att_logp.shape[1]}")
            L = ops.ngram_next(lm, st.tokens, lm_len, None, eos)            # (R, V)
    if L is None and pre_bias is None:
        top_lp, top_i = ops.topk_rows(att_logp, C)                          # (R, C): descending, ties to the lowest id
    else:
        key = att_logp.double()
        if L is not None:
            key = key + lmw * L
        if pre_bias is not None:
            key = key + pre_bias
        _, top_i = ops.topk_rows(key.float(), C)
        top_lp = att_logp.gather(1, top_i)                                  # the exact values, not the key's
    if lm is not None:
        term = L.gather(1, top_i) if L is not None else ops.ngram_next(lm, st.tokens, lm_len, top_i, eos)
        lmv = st.lm.unsqueeze(1) + term
    is_eos = top_i == eos
    att = st.att.unsqueeze(1) + top_lp.double()
    length = st.length.unsqueeze(1) + (~is_eos).long()
    total = (1.0 - lam) * att + beta * length.double()
    ctc = torch.zeros_like(att)
    new_states = None
    if lam > 0:
        hyp_len = torch.where(live, st.length, torch.full_like(st.length, -1))
        last = st.tokens[:, -1] if st.tokens.shape[1] else torch.zeros(R, dtype=torch.int64, device=dev)
        ctc, new_states = ops.ctc_prefix_score(logp, lens, st.state, hyp_len, last, top_i, eos, group=beam, blank=blank, cand_state=cand_state)
        total = (1.0 - lam) * att + lam * ctc + beta * length.double()
    if lm is not None:
        total = total + lmw * lmv
    if context is not None:
        cstate, hits, bias = ops.context_next(context, st.cstate, st.hits, top_i, eos)
        total = total + bias
    total = total.masked_fill(~live.unsqueeze(1), ninf)
    # a finished hypothesis yields itself once, at its slot's first rank; the token appended behind its <eos> is <eos>
    fin = st.finished.unsqueeze(1)
    keep = fin & (torch.arange(C, device=dev).unsqueeze(0) == 0)
    total = torch.where(keep, st.total.unsqueeze(1), total)
    att = torch.where(fin, st.att.unsqueeze(1), att)
    ctc = torch.where(fin, st.ctc.unsqueeze(1), ctc)
    if lm is not None:
        lmv = torch.where(fin, st.lm.unsqueeze(1), lmv)
    if context is not None:
        cstate = torch.where(fin, st.cstate.unsqueeze(1), cstate)
        hits = torch.where(fin, st.hits.unsqueeze(1), hits)
        bias = torch.where(fin, st.bias.unsqueeze(1), bias)
    length = torch.where(fin, st.length.unsqueeze(1), length)
    tok = torch.where(fin, torch.full_like(top_i, eos), top_i)
    # prune: stable, so ties stay in (slot, rank) order; -inf (dropped candidates, missing slots) sorts last
    best, idx = torch.sort(total.view(B, beam * C), dim=1, descending=True, stable=True)
    best, idx = best[:, :beam].reshape(R), idx[:, :beam]
    flat = (idx + torch.arange(B, device=dev).unsqueeze(1) * (beam * C)).reshape(R)
    parents, rank = flat // C, flat % C
    new_tok = tok.reshape(-1).index_select(0, flat)
    tokens = torch.cat((st.tokens.index_select(0, parents), new_tok.unsqueeze(1)), dim=1)
    state = new_states[parents, :, rank] if lam > 0 else None              # (R, Tmax, 2); unread for finished and missing rows
    return BeamState(tokens, parents, att.reshape(-1).index_select(0, flat), ctc.reshape(-1).index_select(0, flat), best,
                     (new_tok == eos) & (best > ninf), length.reshape(-1).index_select(0, flat), state,
                     None if lm is None else lmv.reshape(-1).index_select(0, flat),
                     *((None, None, None) if context is None else
                       tuple(x.reshape(-1).index_select(0, flat) for x in (cstate, hits, bias))))


def joint_beam_search(logp: torch.Tensor, lens: Optional[torch.Tensor], step_fn: Callable, beam: int, C: int, eos: int,
                      ctc_weight: float = 0.3, length_bonus: float = 0.0, max_steps: Optional[int] = None, blank: int = 0, lm=None,
                      lm_weight: float = 0.0, lm_prebeam: bool = True, context=None, context_prebeam: bool = True) -> List[list]:
    """The batched search.  logp (B, Tmax, V) float32 CTC log-probabilities and lens (B) valid frames (or None) on the device;
    step_fn as in the module docstring; 1 <= C <= 64; max_steps defaults to Tmax.
    lm / lm_weight / lm_prebeam: n-gram LM fusion as in the module docstring (None: none).
    -> per utterance [(tokens without <eos>, total, att, ctc, finished)], finished hypotheses first, each group by total; with
    an LM the rows are (tokens, total, att, ctc, finished, lm).
    context / context_prebeam: hotword biasing as in the module docstring (None: none); the rows gain a last element, bias."""
    if not 0.0 <= ctc_weight <= 1.0:
        raise ValueError(f"ctc_weight must lie in [0, 1] (got {ctc_weight})")
    if not 1 <= C <= 64:
        raise ValueError(f"the joint search takes 1..64 candidates per hypothesis (got {C})")
    if beam < 1:
        raise ValueError(f"beam must be >= 1 (got {beam})")
    if lm is not None:
        _check_lm(lm, lm_weight)
    if context is not None:
        _check_context(context)
    B, Tmax, _ = logp.shape
    max_steps = Tmax if max_steps is None else int(max_steps)
    st = initial_state(logp, lens, beam, ctc_weight, blank, lm, context, context_prebeam)
    cand_state = torch.empty(B * beam, Tmax, C, 2, dtype=torch.float64, device=logp.device) if ctc_weight > 0 else None
    for step in range(max_steps):
        if step and bool(((st.total == -float("inf")) | st.finished).all()):   # the one host read of a step
            break
        st = search_step(logp, lens, st, step_fn(st.tokens, st.parents), beam, C, eos, ctc_weight, length_bonus, blank, cand_state,
                         lm, lm_weight, lm_prebeam, context, context_prebeam)
    tokens, total, att, ctc = st.tokens.cpu(), st.total.cpu().tolist(), st.att.cpu().tolist(), st.ctc.cpu().tolist()
    fin, length = st.finished.cpu().tolist(), st.length.cpu().tolist()
    lms = None if lm is None else st.lm.cpu().tolist()
    biases = None if context is None else st.bias.cpu().tolist()
    out = []
    for b in range(B):
        rows = [r for r in range(b * beam, (b + 1) * beam) if total[r] > -float("inf")]
        rows = [r for r in rows if fin[r]] + [r for r in rows if not fin[r]]
        out.append([(tokens[r, : length[r]].tolist(), total[r], att[r], ctc[r], fin[r]) + (() if lm is None else (lms[r],)) +
                    (() if context is None else (biases[r],)) for r in rows])
    return out
