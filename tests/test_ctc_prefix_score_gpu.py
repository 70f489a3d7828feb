"""GPU: the CTC prefix score kernel (oe_ctc_prefix_score, oe_ctc_prefix_score_init) through the C ABI, the joint CTC/attention
search loop (openeat_amd/utils/joint_search.py) with a table-driven attention scorer, and ASRModel.ctc_attention_beam_search on
the tiny Conformer - all against the numpy yardstick ctc_prefix_score_ref.py, which test_ctc_prefix_score_ref.py pins to an
enumeration of every alignment.

Bound on every float64 the device computes with exp / log: 1e-9 * max(1, |x|), as in the device prefix-beam tests; -inf must
sit exactly where the yardstick has it.  Raw calls use a leading dimension above V with log-probability 0 in the padding
columns (an over-read would win every sum), NaN in the frames behind an utterance's length (a read there poisons the row) and
outputs prefilled with a sentinel (a write that should not happen shows).

The file is not named test_gpu_*: conftest.py orders those files by a fixed list that test_host_logic.py holds complete."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_prefix_score_ref as ref  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.utils import joint_search as js  # noqa: E402

DEV = "cuda"
SENT = 777.0
NEG = -math.inf


def assert_close(got, want, what):
    """got, want: float64 arrays; -inf exactly where the yardstick has it, the rest within 1e-9 * max(1, |x|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), (what, "-inf pattern", got, want)
    assert not np.isnan(got).any(), (what, "NaN")
    err = np.abs(got[~inf] - want[~inf])
    tol = 1e-9 * np.maximum(1.0, np.abs(want[~inf]))
    assert (err <= tol).all(), (what, float(err.max()) if err.size else 0.0)


def host_log_softmax(rng, shape, scale=1.5):
    x = (rng.randn(*shape) * scale).astype(np.float64)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def raw_init(logp, lens, B, Tmax, V, ldv, group, state):
    hip.check(hip.lib().oe_ctc_prefix_score_init(hip.ptr(logp), hip.ptr(lens), B, Tmax, V, ldv, group, 0, hip.ptr(state), hip.stream()),
              "oe_ctc_prefix_score_init")


def raw_score(logp, lens, B, Tmax, V, ldv, group, state, hyp_len, last, cand, C, eos, psi, cand_state):
    hip.check(hip.lib().oe_ctc_prefix_score(hip.ptr(logp), hip.ptr(lens), B, Tmax, V, ldv, group, hip.ptr(state), hip.ptr(hyp_len),
                                            hip.ptr(last), hip.ptr(cand), C, 0, eos, hip.ptr(psi), hip.ptr(cand_state), hip.stream()),
              "oe_ctc_prefix_score")


@pytest.mark.parametrize("B,Tmax,V,group,C,lens", [(3, 7, 6, 2, 3, [7, 0, 1]), (2, 23, 12, 4, 12, [20, 0]), (2, 70, 80, 3, 64, [70, 1])])
def test_kernel_against_the_yardstick_along_hypothesis_chains(B, Tmax, V, group, C, lens):
    """Random hypothesis chains of depth 4: at every depth each row scores C candidates - the blank, <eos>, an id outside
    the vocabulary and the parent's last token among them - and is extended by one of them (by its own last token every other
    time, so that hypotheses with repeated tokens are scored) on the device's own state.  Row 1 is a slot that does not exist."""
    rng = np.random.RandomState(1000 + Tmax)
    eos, ldv, R, missing = V - 1, V + 3, B * group, 1
    y = np.zeros((B, Tmax, ldv), dtype=np.float32)
    y[:, :, :V] = host_log_softmax(rng, (B, Tmax, V))
    for u in range(B):
        y[u, lens[u]:] = np.nan
    y64 = y[:, :, :V].astype(np.float64)
    logp = torch.from_numpy(y).to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    T = [lens[r // group] for r in range(R)]

    state = torch.full((R, Tmax, 2), SENT, dtype=torch.float64, device=DEV)
    raw_init(logp, lens_d, B, Tmax, V, ldv, group, state)
    got = state.cpu().numpy()
    want_state = [ref.empty_state(y64[r // group], T[r]) for r in range(R)]
    for r in range(R):
        assert_close(got[r, :T[r]], want_state[r], f"empty state of row {r}")
        assert (got[r, T[r]:] == SENT).all(), f"row {r}: the empty state was written behind the utterance's length"

    g = [() for _ in range(R)]
    seen = set()
    for depth in range(4):
        cand = rng.randint(1, V - 1, size=(R, C))
        ext = [0] * R
        for r in range(R):
            specials = [("blank", 0), ("eos", eos), ("range", V + 2 if (r + depth) % 2 else -1),
                        ("last", g[r][-1] if g[r] else int(cand[r, 0]))]
            for i in range(min(4, C - 1)):
                kind, tok = specials[(r + depth + i) % 4]
                cand[r, 1 + i] = tok
                seen.add(kind if kind != "last" or g[r] else "first")
                if kind == "last" and g[r] and (r + depth) % 2 == 0:
                    ext[r] = 1 + i
        hyp_len = [-1 if r == missing else len(g[r]) for r in range(R)]
        last = [g[r][-1] if g[r] else int(cand[r, 0]) for r in range(R)]      # what an empty hypothesis names must not be used
        hl_d = torch.tensor(hyp_len, dtype=torch.int32, device=DEV)
        last_d = torch.tensor(last, dtype=torch.int32, device=DEV)
        cand_d = torch.from_numpy(cand.astype(np.int32)).to(DEV)
        psi = torch.full((R, C), SENT, dtype=torch.float64, device=DEV)
        psi_only = torch.full((R, C), SENT, dtype=torch.float64, device=DEV)
        cs = torch.full((R, Tmax, C, 2), SENT, dtype=torch.float64, device=DEV)
        raw_score(logp, lens_d, B, Tmax, V, ldv, group, state, hl_d, last_d, cand_d, C, eos, psi, cs)
        raw_score(logp, lens_d, B, Tmax, V, ldv, group, state, hl_d, last_d, cand_d, C, eos, psi_only, None)
        torch.cuda.synchronize()
        assert torch.equal(psi.view(torch.int64), psi_only.view(torch.int64)), "psi differs when no states are asked for"
        psi_h, cs_h = psi.cpu().numpy(), cs.cpu().numpy()
        for r in range(R):
            if r == missing:
                assert np.isneginf(psi_h[r]).all() and (cs_h[r] == SENT).all(), "the missing slot"
                continue
            assert (cs_h[r, T[r]:] == SENT).all(), f"row {r}: states written behind the utterance's length"
            new = None
            for j in range(C):
                c = int(cand[r, j])
                want_psi, n = ref.prefix_score(y64[r // group], T[r], want_state[r], g[r], c, eos)
                assert_close(psi_h[r, j], want_psi, f"psi depth {depth} row {r} candidate {j} = {c} after {g[r]}")
                if n is None:
                    assert (cs_h[r, :, j] == SENT).all(), f"row {r} candidate {c}: a state where none is produced"
                else:
                    assert_close(cs_h[r, :T[r], j], n, f"state depth {depth} row {r} candidate {j} = {c} after {g[r]}")
                if j == ext[r]:
                    new = n
            # extend on the device's own state; with no frames there is no state and the (empty) yardstick state stays
            state[r] = cs[r, :, ext[r], :]
            g[r] = g[r] + (int(cand[r, ext[r]]),)
            if new is not None:
                want_state[r] = new
    assert seen >= {"blank", "eos", "range", "last", "first"}
    assert any(len(h) >= 2 and h[-1] == h[-2] for h in g), "no hypothesis with a repeated token was scored"


# ---- the search loop with a table-driven attention scorer ------------------------------------------------------------
def make_case_host(B, Tmax, V, seed, eos_first=0.0, eos_rest=0.0, blank=0.0, att_scale=2.0):
    """CTC log-probabilities (B, Tmax, V) and an attention table (B, Tmax + 1, V + 1, V) indexed by (utterance, step, last
    token + 1) as float32 numpy arrays, log-softmaxed on the host in float64 and rounded once: the kernel and the yardstick
    read the very same float32 values, and what a seed gives can be examined without a device.  eos_first / eos_rest are
    added to the <eos> logit of the table's first / later steps, blank to the CTC blank logit."""
    rng = np.random.RandomState(seed)
    ctc = rng.randn(B, Tmax, V) * 1.5
    ctc[..., 0] += blank
    tab = rng.randn(B, Tmax + 1, V + 1, V) * att_scale
    tab[:, 0, :, V - 1] += eos_first
    tab[:, 1:, :, V - 1] += eos_rest
    def lsm(x):
        x = x - x.max(-1, keepdims=True)
        return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
    return lsm(ctc), lsm(tab)


def to_device(y, tab, lens):
    return torch.from_numpy(y).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), torch.from_numpy(tab).to(DEV)


def table_step_fn(table, beam):
    R, steps = table.shape[0] * beam, table.shape[1] - 1
    utt = torch.arange(R, device=DEV) // beam

    def step_fn(tokens, parents):
        n = tokens.shape[1]
        last = tokens[:, -1] + 1 if n else torch.zeros(R, dtype=torch.int64, device=DEV)
        return table[utt, min(n, steps), last].contiguous()
    return step_fn


def yardstick_search(y, tab, lens, beam, C, lam, beta, max_steps):
    y64, V, steps = y.astype(np.float64), y.shape[2], tab.shape[1] - 1
    out = []
    for u in range(y.shape[0]):
        att = lambda g, u=u: tab[u, min(len(g), steps), (g[-1] + 1) if g else 0]     # noqa: E731
        out.append(ref.joint_search(y64[u], int(lens[u]), att, V - 1, beam, C, lam, beta, max_steps))
    return out


def compare_search(got, want, what):
    for u, (nb, (ref_nb, gap)) in enumerate(zip(got, want)):
        assert gap >= 1e-8, (what, u, "the yardstick's totals are too close to order", gap)
        assert [h[0] for h in nb] == [h[0] for h in ref_nb], (what, u, nb, ref_nb)
        assert [h[4] for h in nb] == [h[4] for h in ref_nb], (what, u)
        for k, name in ((1, "total"), (2, "att"), (3, "ctc")):
            assert_close([h[k] for h in nb], [h[k] for h in ref_nb], f"{what} utterance {u} {name}")


def run_both(y, tab, lens, beam, C, lam, beta, max_steps, what):
    logp, lens_d, table = to_device(y, tab, lens)
    got = js.joint_beam_search(logp, lens_d, table_step_fn(table, beam), beam, C, y.shape[2] - 1, lam, beta, max_steps=max_steps)
    compare_search(got, yardstick_search(y, tab, lens, beam, C, lam, beta, y.shape[1] if max_steps is None else max_steps), what)
    return got


# (B, Tmax, V, lens, seed): the seeds were examined on the host - the smallest gap between neighbouring totals over all the
# prunings of all the cases below is far above the 1e-8 that compare_search asserts
SHAPES = {"small": (3, 7, 6, [7, 0, 1], 11), "mid": (2, 23, 12, [20, 0], 12)}
SURVIVOR = dict(B=2, Tmax=7, V=6, lens=[7, 6], seed=21, beam=3, C=6, kw=dict(eos_first=4.0, eos_rest=-12.0, blank=3.0, att_scale=0.5))
LIMIT = dict(B=2, Tmax=7, V=6, lens=[7, 5], seed=31, beam=3, C=3, kw=dict(eos_first=-30.0, eos_rest=-30.0))


@pytest.mark.parametrize("beam", [1, 3, 4])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_search_loop_against_the_yardstick(shape, lam, beam):
    """n-best lists, their order and the finished flags exactly, scores within the bound; beta in {0, 0.5}, C in {1, 3, V}."""
    B, Tmax, V, lens, seed = SHAPES[shape]
    y, tab = make_case_host(B, Tmax, V, seed)
    for beta in (0.0, 0.5):
        for C in (1, 3, V):
            run_both(y, tab, lens, beam, C, lam, beta, None, f"{shape} lam={lam} beam={beam} beta={beta} C={C}")


def test_a_finished_hypothesis_survives_beside_unfinished_ones():
    """<eos> is likely at the first step and all but impossible afterwards, and the CTC posterior leans to the blank: the
    hypothesis that ended at once keeps its slot and its scores, step after step, while the other slots go on growing."""
    c = SURVIVOR
    y, tab = make_case_host(c["B"], c["Tmax"], c["V"], c["seed"], **c["kw"])
    first = None
    for max_steps in (1, 2, 3, 4, 5):
        got = run_both(y, tab, c["lens"], c["beam"], c["C"], 0.3, 0.0, max_steps, f"max_steps={max_steps}")
        for nb in got:
            assert [h[4] for h in nb] == [True, False, False] and nb[0][0] == [], nb
            assert all(len(h[0]) == max_steps for h in nb[1:]), nb
        first = first or [nb[0] for nb in got]
        assert [nb[0] for nb in got] == first, "the finished hypothesis changed while it waited"


def test_the_step_limit_ends_a_search_with_nothing_finished():
    c = LIMIT
    y, tab = make_case_host(c["B"], c["Tmax"], c["V"], c["seed"], **c["kw"])
    got = run_both(y, tab, c["lens"], c["beam"], c["C"], 0.3, 0.5, 3, "step limit")
    for nb in got:
        assert len(nb) == c["beam"] and not any(h[4] for h in nb) and all(len(h[0]) == 3 for h in nb), nb


def test_one_step_is_capturable():
    """Score + prune of one step under torch.cuda.graph, replayed twice: the same survivors and scores as the eager step."""
    B, Tmax, V, lens, seed = SHAPES["mid"]
    beam, C, lam, beta = 3, 5, 0.3, 0.5
    logp, lens_d, table = to_device(*make_case_host(B, Tmax, V, seed), lens)
    fn = table_step_fn(table, beam)
    st = js.initial_state(logp, lens_d, beam, lam)
    for _ in range(2):
        st = js.search_step(logp, lens_d, st, fn(st.tokens, st.parents), beam, C, V - 1, lam, beta)
    att_logp = fn(st.tokens, st.parents)
    eager = js.search_step(logp, lens_d, st, att_logp, beam, C, V - 1, lam, beta)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = js.search_step(logp, lens_d, st, att_logp, beam, C, V - 1, lam, beta)
    for _ in range(2):
        for t in (out.tokens, out.total, out.att, out.ctc, out.state):
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        alive = (eager.total > NEG).cpu()
        assert alive.any()
        assert torch.equal(out.tokens.cpu()[alive], eager.tokens.cpu()[alive])
        assert torch.equal(out.parents, eager.parents) and torch.equal(out.finished, eager.finished)
        for a, b in ((out.total, eager.total), (out.att, eager.att), (out.ctc, eager.ctc)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        live = (alive & ~eager.finished.cpu()).nonzero().flatten().tolist()
        for r in live:
            T = lens[r // beam]
            assert torch.equal(out.state[r, :T].view(torch.int64), eager.state[r, :T].view(torch.int64))


# ---- end to end on the tiny Conformer --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_conformer():
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    return model.to(DEV).eval(), g["in"]["feats"][:2].contiguous().to(DEV), g["in"]["flen"][:2].to(DEV), meta


def test_model_beam_one_without_ctc_is_recognize(tiny_conformer):
    model, feats, flen, meta = tiny_conformer
    with torch.no_grad():
        rec = model.recognize(feats, flen, beam_size=1).tolist()
    got = model.ctc_attention_beam_search(feats, flen, beam_size=1, ctc_weight=0.0)
    want = [row[: row.index(model.eos)] if model.eos in row else row for row in rec]
    assert got == want and all(len(t) > 0 for t in got)


def test_model_hypotheses_rescore_on_their_own(tiny_conformer):
    """beam 3, ctc_weight 0.3: every (tokens, total, att, ctc) against one teacher-forced decoder pass (a wrongly ordered
    decoder cache breaks this), the yardstick's CTC score of the tokens, and the mix of the two.  The list does not say
    whether a hypothesis ended in <eos>, and the two readings differ in both scores (the log-probability of <eos> resp. the
    full likelihood in place of the prefix score): all three numbers must fit one reading, finished ones first."""
    from openeat_amd.utils.mask import subsequent_mask
    model, feats, flen, meta = tiny_conformer
    lam, V, eos = 0.3, meta["V"], model.eos
    res = model.ctc_attention_beam_search(feats, flen, beam_size=3, ctc_weight=lam, nbest=True, max_len=8)
    with torch.no_grad():
        enc, enc_mask, _ = model._encode(feats, flen)
        logp = ops.log_softmax_rows(model.ctc.logits(enc)).cpu().numpy().astype(np.float64)
        lens = enc_mask.squeeze(1).sum(1).tolist()
        assert len(res) == 2
        for b, nb in enumerate(res):
            assert len(nb) == 3
            readings = []
            for tokens, total, att, ctc in nb:
                L = len(tokens) + 1
                ys = torch.tensor([[model.sos] + tokens], dtype=torch.long, device=DEV)
                mask = subsequent_mask(L, device=DEV).unsqueeze(0)
                logits, _, _ = model.decoder(enc[b:b + 1], enc_mask[b:b + 1], ys, ys, mask)
                logits = logits[0].double().cpu()
                lp = torch.log_softmax(logits, dim=-1)
                bound = 2 * L * (1e-4 + 2e-4 * float(logits.abs().max()))
                att_open = float(sum(lp[j, w] for j, w in enumerate(tokens)))
                T = int(lens[b])
                ctc_open = 0.0 if not tokens else ref.prefix_score(logp[b], T, ref.state_of(logp[b], T, tokens[:-1], eos),
                                                                   tuple(tokens[:-1]), tokens[-1], eos)[0]
                fits = []
                for fin, a, k in ((False, att_open, ctc_open),
                                  (True, att_open + float(lp[L - 1, eos]), ref.full_likelihood(logp[b], T, tokens, eos))):
                    ok_ctc = (k == ctc) if k == NEG or ctc == NEG else abs(ctc - k) <= 1e-9 * max(1.0, abs(k))
                    mix = (1 - lam) * att + lam * ctc
                    if abs(att - a) <= bound and ok_ctc and abs(total - mix) <= 1e-9 * max(1.0, abs(mix)):
                        fits.append(fin)
                assert len(fits) == 1, (b, tokens, total, att, ctc, att_open, ctc_open, bound)
                readings.append(fits[0])
            assert readings == sorted(readings, reverse=True), "finished hypotheses come first"
            by_group = [[h[1] for h, f in zip(nb, readings) if f == fin] for fin in (True, False)]
            assert all(t == sorted(t, reverse=True) for t in by_group)
    best = model.ctc_attention_beam_search(feats, flen, beam_size=3, ctc_weight=lam, max_len=8)
    assert best == [nb[0][0] for nb in res]


def test_model_refuses_what_it_cannot_decode(tiny_conformer):
    from openeat_amd.models.asr_model import ASRModel
    model, feats, flen, meta = tiny_conformer
    for kw in (dict(ctc_weight=-0.1), dict(ctc_weight=1.5), dict(ctc_candidates=0), dict(ctc_candidates=65)):
        with pytest.raises(ValueError):
            model.ctc_attention_beam_search(feats, flen, beam_size=2, **kw)
    kwargs = dict(meta["kwargs"], ctc_weight=1.0)
    ctc_only = ASRModel(80, meta["V"], **kwargs)
    with pytest.raises(ValueError, match="decoder"):
        ctc_only.ctc_attention_beam_search(feats, flen, beam_size=2)
