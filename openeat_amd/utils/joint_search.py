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
(slot, rank) tie order.  The loop reads one flag per step on the host, the all-finished test, as ASRModel.recognize does."""
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


def initial_state(logp: torch.Tensor, lens: Optional[torch.Tensor], beam: int, ctc_weight: float, blank: int = 0) -> BeamState:
    """The one empty hypothesis per utterance in slot 0; the other slots do not exist yet."""
    B, dev = logp.shape[0], logp.device
    R = B * beam
    total = torch.full((B, beam), -float("inf"), dtype=torch.float64, device=dev)
    total[:, 0] = 0.0
    zeros = torch.zeros(R, dtype=torch.float64, device=dev)
    state = ops.ctc_prefix_score_init(logp, lens, group=beam, blank=blank) if ctc_weight > 0 else None
    return BeamState(torch.zeros(R, 0, dtype=torch.int64, device=dev), None, zeros, zeros.clone(), total.view(R),
                     torch.zeros(R, dtype=torch.bool, device=dev), torch.zeros(R, dtype=torch.int64, device=dev), state)


def search_step(logp: torch.Tensor, lens: Optional[torch.Tensor], st: BeamState, att_logp: torch.Tensor, beam: int, C: int, eos: int,
                ctc_weight: float, length_bonus: float, blank: int = 0, cand_state: Optional[torch.Tensor] = None) -> BeamState:
    """One step: candidates, their CTC prefix scores, the prune.  att_logp (R, V) float32 for st's rows.  No host read."""
    dev = logp.device
    R = st.total.shape[0]
    B = R // beam
    lam, beta = float(ctc_weight), float(length_bonus)
    ninf = -float("inf")
    alive = st.total > ninf
    live = alive & ~st.finished
    top_lp, top_i = ops.topk_rows(att_logp, C)                              # (R, C): descending, ties to the lowest id
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
    total = total.masked_fill(~live.unsqueeze(1), ninf)
    # a finished hypothesis yields itself once, at its slot's first rank; the token appended behind its <eos> is <eos>
    fin = st.finished.unsqueeze(1)
    keep = fin & (torch.arange(C, device=dev).unsqueeze(0) == 0)
    total = torch.where(keep, st.total.unsqueeze(1), total)
    att = torch.where(fin, st.att.unsqueeze(1), att)
    ctc = torch.where(fin, st.ctc.unsqueeze(1), ctc)
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
                     (new_tok == eos) & (best > ninf), length.reshape(-1).index_select(0, flat), state)


def joint_beam_search(logp: torch.Tensor, lens: Optional[torch.Tensor], step_fn: Callable, beam: int, C: int, eos: int,
                      ctc_weight: float = 0.3, length_bonus: float = 0.0, max_steps: Optional[int] = None, blank: int = 0) -> List[list]:
    """The batched search.  logp (B, Tmax, V) float32 CTC log-probabilities and lens (B) valid frames (or None) on the device;
    step_fn as in the module docstring; 1 <= C <= 64; max_steps defaults to Tmax.
    -> per utterance [(tokens without <eos>, total, att, ctc, finished)], finished hypotheses first, each group by total."""
    if not 0.0 <= ctc_weight <= 1.0:
        raise ValueError(f"ctc_weight must lie in [0, 1] (got {ctc_weight})")
    if not 1 <= C <= 64:
        raise ValueError(f"the joint search takes 1..64 candidates per hypothesis (got {C})")
    if beam < 1:
        raise ValueError(f"beam must be >= 1 (got {beam})")
    B, Tmax, _ = logp.shape
    max_steps = Tmax if max_steps is None else int(max_steps)
    st = initial_state(logp, lens, beam, ctc_weight, blank)
    cand_state = torch.empty(B * beam, Tmax, C, 2, dtype=torch.float64, device=logp.device) if ctc_weight > 0 else None
    for step in range(max_steps):
        if step and bool(((st.total == -float("inf")) | st.finished).all()):   # the one host read of a step
            break
        st = search_step(logp, lens, st, step_fn(st.tokens, st.parents), beam, C, eos, ctc_weight, length_bonus, blank, cand_state)
    tokens, total, att, ctc = st.tokens.cpu(), st.total.cpu().tolist(), st.att.cpu().tolist(), st.ctc.cpu().tolist()
    fin, length = st.finished.cpu().tolist(), st.length.cpu().tolist()
    out = []
    for b in range(B):
        rows = [r for r in range(b * beam, (b + 1) * beam) if total[r] > -float("inf")]
        rows = [r for r in rows if fin[r]] + [r for r in rows if not fin[r]]
        out.append([(tokens[r, : length[r]].tolist(), total[r], att[r], ctc[r], fin[r]) for r in rows])
    return out
