"""GPU: n-gram LM fusion in the joint CTC/attention beam search - the kernel behind it (oe_ngram_next) through the C ABI, the
search loop (openeat_amd/utils/joint_search.py) with a table-driven attention scorer against the yardstick
joint_lm_search_ref.py, and ASRModel.ctc_attention_beam_search with an LM on the tiny Conformer.

The kernel's terms are compared bit for bit with oe_ngram_score's per-token output for hypothesis + candidate and with
NgramLM.full_scores on the host (both add the same float32 values in float64 in the same order), and within
1e-9 * max(1, |x|) with ngram_ref.RefLM, which adds them in the opposite order.  The search is compared with the yardstick
exactly in its tokens, order and finished flags and within the same bound in its scores; that is sound because the
yardstick's totals and pre-selection keys keep a distance (asserted here, examined on the host by
test_joint_lm_search_ref.py) far above what the last bit of a term can move.

The file is not named test_gpu_*: conftest.py orders those files by a fixed list that test_host_logic.py holds complete."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import joint_lm_search_ref as R  # noqa: E402
import ngram_ref  # noqa: E402
from openeat_amd import hip, ops  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402
from openeat_amd.utils import joint_search as js  # noqa: E402

DEV = "cuda"
SENT = 777.0
NEG = -math.inf


def bits(t):
    return t.contiguous().view(torch.int64)


def assert_close(got, want, what):
    """-inf exactly where the yardstick has it, the rest within 1e-9 * max(1, |x|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), (what, "-inf pattern", got, want)
    assert not np.isnan(got).any(), (what, "NaN")
    err = np.abs(got[~inf] - want[~inf])
    tol = 1e-9 * np.maximum(1.0, np.abs(want[~inf]))
    assert (err <= tol).all(), (what, float(err.max()) if err.size else 0.0)


# ---- the kernel through the C ABI ------------------------------------------------------------------------------------
def raw_next(lm, tokens, ld, lens, R_, cand, C, eos_tok):
    """-> out (R, C) float64; the buffer is a row longer than (R, C) and prefilled: every entry inside must be written,
    nothing behind."""
    buf = torch.full((R_ * C + C,), SENT, dtype=torch.float64, device=DEV)
    hip.check(hip.lib().oe_ngram_next(hip.ngram_model(lm, DEV), hip.ptr(tokens), ld, hip.ptr(lens), R_, hip.ptr(cand), C, eos_tok,
                                      hip.ptr(buf), hip.stream()), "oe_ngram_next")
    torch.cuda.synchronize()
    assert (buf[R_ * C:] == SENT).all(), "written behind (R, C)"
    out = buf[: R_ * C].view(R_, C)
    assert not (out == SENT).any(), "an entry of (R, C) was not written"
    return out


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_kernel_bit_for_bit_against_score_kernel_and_host(tmp_path, order):
    """Rows of 0, 1, order-2, order-1, order and order+3 tokens, a missing slot and a length above ld; behind every length
    the row holds ids of real words.  Full form with V in {6, 50, 300} (300 crosses a slice of 256 candidates), candidate
    form with C in {1, 7, 64, 70} whose candidates hold the eos_tok, the blank, -5, V + 3, a token mapped to <unk> and a
    duplicate.  The eos_tok's own string is a real word: as a candidate it must score </s> all the same."""
    rng = np.random.default_rng(100 + order)
    for V in (6, 50, 300):
        nw = V - 3
        path = str(tmp_path / f"next_{V}.arpa")
        words = ngram_ref.random_arpa(path, order, nw, 30 * nw, rng, with_unk=(V != 50))
        t2c = ["<blank>"] + words + ["oov", words[0]]             # token V-2 is unmapped, token V-1 is the eos_tok
        eos_tok = V - 1
        lm, ref = NgramLM(path, t2c), ngram_ref.RefLM(path)
        assert lm.order == order and len(lm.tok2word) == V
        ld = order + 4
        raw_lens = [0, 1, max(order - 2, 0), order - 1, order, order + 3, -1, ld + 5]
        nR, missing = len(raw_lens), 6
        eff = [min(n, ld) for n in raw_lens]
        tokens = rng.integers(1, V - 2, size=(nR, ld)).astype(np.int32)          # real words everywhere, behind the lengths too
        for r in range(nR):                                                       # inside: also the blank, the unmapped one,
            for i, t in enumerate((0, V - 2, V - 1, V + 3, -5)):                  # the eos id (a word there) and ids out of range
                if eff[r] > i + 1 and (r + i) % 2:
                    tokens[r, (r + i) % eff[r]] = t
        tok_d = torch.from_numpy(tokens).to(DEV)
        len_d = torch.tensor(raw_lens, dtype=torch.int32, device=DEV)
        live = [r for r in range(nR) if r != missing]

        def word(t):
            return t2c[t] if 0 <= t < V and (t2c[t],) in ref.grams else "<unk>"

        def sentence(r):
            return " ".join(t2c[t] if 0 <= t < V else "oov" for t in tokens[r, :eff[r]])

        memo = {}

        def host(r, t):
            """(NgramLM.full_scores' term, RefLM's) of token t after row r."""
            key = (r, "</s>" if t == eos_tok else word(t))
            if key not in memo:
                seq = ["<s>"] + [word(x) for x in tokens[r, :eff[r]]]
                h = tuple(seq[max(0, len(seq) - (order - 1)):]) if order > 1 else ()
                if t == eos_tok:
                    memo[key] = (lm.full_scores(sentence(r), True, True)[-1][0], ref.p("</s>", h)[0])
                else:
                    s = (sentence(r) + " " + (t2c[t] if 0 <= t < V else "oov")).strip()
                    memo[key] = (lm.full_scores(s, True, False)[-1][0], ref.p(word(t), h)[0])
            return memo[key]

        def by_score_kernel(cand):
            """oe_ngram_score(per_token) on hypothesis + candidate, one row per (row, candidate): tok_logp[., len]; for the
            eos_tok the </s> term of the hypothesis scored with eos = 1."""
            C = cand.shape[1]
            rows = np.zeros((nR * C, ld + 1), dtype=np.int32)
            lens = np.zeros(nR * C, dtype=np.int32)
            for r in range(nR):
                for j in range(C):
                    n = max(eff[r], 0)
                    rows[r * C + j, :n] = tokens[r, :n]
                    rows[r * C + j, n] = cand[r, j]
                    lens[r * C + j] = eff[r] + 1 if r != missing else -1
            _, lp, _ = ops.ngram_score(lm, torch.from_numpy(rows).to(DEV), torch.from_numpy(lens).to(DEV), bos=True, eos=False,
                                       per_token=True)
            pos = torch.tensor([max(eff[r], 0) for r in range(nR) for _ in range(C)], device=DEV)
            want = lp.gather(1, pos.unsqueeze(1)).view(nR, C).clone()
            _, lp_e, _ = ops.ngram_score(lm, tok_d, torch.tensor(eff, dtype=torch.int32, device=DEV), bos=True, eos=True, per_token=True)
            ends = lp_e.gather(1, torch.tensor([max(n, 0) for n in eff], device=DEV).unsqueeze(1))          # (R, 1)
            return torch.where(torch.from_numpy(cand == eos_tok).to(DEV), ends.expand(nR, C), want)

        def check(out, cand, what):
            got = out.cpu().numpy()
            assert np.isneginf(got[missing]).all() and np.isfinite(got[live]).all(), (what, "-inf sits on the missing slot's row only")
            want = by_score_kernel(cand)
            assert torch.equal(bits(out[live]), bits(want[live])), (what, "differs from oe_ngram_score's tok_logp")
            for r in live:
                for j in range(cand.shape[1]):
                    full, yard = host(r, int(cand[r, j]))
                    assert got[r, j] == full, (what, r, j, int(cand[r, j]), got[r, j], full)
                    assert abs(got[r, j] - yard) <= 1e-9 * max(1.0, abs(yard)), (what, r, j, got[r, j], yard)

        every = np.tile(np.arange(V, dtype=np.int32), (nR, 1))
        full = raw_next(lm, tok_d, ld, len_d, nR, None, V, eos_tok)
        check(full, every, f"order {order} V {V} full form")
        # eos_tok = -1: no token is </s>, the token V-1 scores its own word - and only that column changes
        plain = raw_next(lm, tok_d, ld, len_d, nR, None, V, -1)
        assert torch.equal(bits(plain[:, :V - 1]), bits(full[:, :V - 1]))
        assert torch.equal(bits(plain[live, V - 1]), bits(full[live, 1])) and not torch.equal(bits(plain[live, V - 1]), bits(full[live, V - 1]))

        specials = [eos_tok, 0, -5, V + 3, V - 2]
        for C in (1, 7, 64, 70):
            cand = rng.integers(1, V - 2, size=(nR, C)).astype(np.int32)
            for r in range(nR):
                for i, t in enumerate(specials):
                    if C == 1:
                        if i == r % len(specials):
                            cand[r, 0] = t
                    elif (r + i) % C != C - 1:
                        cand[r, (r + i) % C] = t
                if C > 1:
                    cand[r, C - 1] = cand[r, 0]                                  # a duplicate
            out = raw_next(lm, tok_d, ld, len_d, nR, torch.from_numpy(cand).to(DEV), C, eos_tok)
            check(out, cand, f"order {order} V {V} C {C}")
            inside = torch.from_numpy((cand >= 0) & (cand < V)).to(DEV)
            shared = full.gather(1, torch.from_numpy(np.clip(cand, 0, V - 1)).to(DEV).long())
            assert torch.equal(bits(out[inside]), bits(shared[inside])), "the candidate form and the full form differ on a shared token"
            unk = full[:, 0:1].expand(nR, C)                                     # the blank is <unk>, as every id out of range
            assert torch.equal(bits(out[~inside]), bits(unk[~inside]))
            if C > 1:
                assert torch.equal(bits(out[:, C - 1]), bits(out[:, 0]))
        # through ops: int64 tensors as the search passes them, both forms
        cand = torch.from_numpy(cand).to(DEV).long()
        assert torch.equal(bits(ops.ngram_next(lm, tok_d.long(), len_d.long(), cand, eos_tok)), bits(out))
        assert torch.equal(bits(ops.ngram_next(lm, tok_d.long(), len_d.long(), None, eos_tok)), bits(full))
        assert torch.equal(bits(ops.ngram_next(lm, tok_d.long(), len_d.long())), bits(plain))
        # no tokens at all: every row is <s> alone
        none = ops.ngram_next(lm, tok_d[:, :0], torch.zeros(nR, dtype=torch.int32, device=DEV), None, eos_tok)
        assert torch.equal(bits(none), bits(full[0:1].expand(nR, V)))


def test_ops_ngram_next_refuses_what_it_cannot_score(tmp_path):
    lm = NgramLM(*R.make_lm(tmp_path, 6, 2, 1))
    tokens, lens = torch.zeros(2, 3, dtype=torch.int32, device=DEV), torch.tensor([3, 3], dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="CUDA"):
        ops.ngram_next(lm, tokens, lens.cpu())
    with pytest.raises(TypeError, match="CUDA"):
        ops.ngram_next(lm, tokens, lens, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(TypeError, match="integer"):
        ops.ngram_next(lm, tokens.float(), lens)
    with pytest.raises(TypeError, match="integer"):
        ops.ngram_next(lm, tokens, lens, torch.zeros(3, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.ngram_next(lm, tokens, lens, torch.zeros(2, 0, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.ngram_next(lm, tokens, lens, eos=6)


# ---- the search loop with a table-driven attention scorer ------------------------------------------------------------
def to_device(y, tab, lens):
    return torch.from_numpy(y).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), torch.from_numpy(tab).to(DEV)


def table_step_fn(table, beam):
    R_, steps = table.shape[0] * beam, table.shape[1] - 1
    utt = torch.arange(R_, device=DEV) // beam

    def step_fn(tokens, parents):
        n = tokens.shape[1]
        last = tokens[:, -1] + 1 if n else torch.zeros(R_, dtype=torch.int64, device=DEV)
        return table[utt, min(n, steps), last].contiguous()
    return step_fn


def compare_search(got, want, what):
    for u, (nb, (ref_nb, gap, key_gap)) in enumerate(zip(got, want)):
        assert gap >= R.TOTAL_GAP, (what, u, "the yardstick's totals are too close to order", gap)
        assert key_gap >= R.KEY_GAP, (what, u, "the yardstick's pre-selection keys are too close to cut", key_gap)
        assert [h[0] for h in nb] == [h[0] for h in ref_nb], (what, u, nb, ref_nb)
        assert [h[4] for h in nb] == [h[4] for h in ref_nb], (what, u)
        for k, name in ((1, "total"), (2, "att"), (3, "ctc"), (5, "lm")):
            assert_close([h[k] for h in nb], [h[k] for h in ref_nb], f"{what} utterance {u} {name}")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """The tables of every shape on the host and the device, and the LM of every (V, order) as (NgramLM, PrefixLM)."""
    tmp = tmp_path_factory.mktemp("joint_lm")
    tables, lms = {}, {}
    specs = dict(R.SHAPES, survivor=(R.SURVIVOR["B"], R.SURVIVOR["Tmax"], R.SURVIVOR["V"], R.SURVIVOR["lens"], R.SURVIVOR["seed"]))
    for name, (B, Tmax, V, lens, seed) in specs.items():
        y, tab = R.make_case_host(B, Tmax, V, seed, **(R.SURVIVOR["kw"] if name == "survivor" else {}))
        tables[name] = (y, tab, lens) + to_device(y, tab, lens)
        for order in R.ORDERS:
            if (V, order) not in lms:
                path, t2c = R.make_lm(tmp, V, order, R.LM_SEED)
                lms[V, order] = (NgramLM(path, t2c), R.prefix_lm(path, t2c))
    return tables, lms


@pytest.mark.parametrize("beam", R.BEAMS)
@pytest.mark.parametrize("lam", R.LAMS)
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_search_loop_against_the_yardstick(cases, shape, lam, beam):
    """lm_weight in {0.5, 2.0} (with C = 3, beta = 0 resp. C = 4, beta = 0.5), both pre-selection modes, ARPA orders 2 and 4:
    n-best lists, their order and the finished flags exactly, total, att, ctc and lm within the bound."""
    tables, lms = cases
    y, tab, lens, logp, lens_d, table = tables[shape]
    V, Tmax = y.shape[2], y.shape[1]
    ran = 0
    for s, l, b, w, pre, order in R.search_cases():
        if (s, l, b) != (shape, lam, beam):
            continue
        C, beta = R.WEIGHTS[w]
        lm, plm = lms[V, order]
        got = js.joint_beam_search(logp, lens_d, table_step_fn(table, beam), beam, C, V - 1, lam, beta, None, 0, lm, w, pre)
        assert all(len(h) == 6 for nb in got for h in nb)
        compare_search(got, R.yardstick(y, tab, lens, plm, beam, C, lam, beta, Tmax, w, pre),
                       f"{shape} lam={lam} beam={beam} lm_weight={w} prebeam={pre} order={order}")
        ran += 1
    assert ran == 8


@pytest.mark.parametrize("lm_prebeam", [True, False])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_weight_zero_is_the_search_without_an_lm_by_bit(cases, shape, lm_prebeam):
    tables, lms = cases
    y, tab, lens, logp, lens_d, table = tables[shape]
    V = y.shape[2]
    for lam in R.LAMS:
        for beam, C, beta in ((1, 3, 0.0), (3, 4, 0.5), (3, V, 0.0)):
            fn = table_step_fn(table, beam)
            want = js.joint_beam_search(logp, lens_d, fn, beam, C, V - 1, lam, beta)
            got = js.joint_beam_search(logp, lens_d, fn, beam, C, V - 1, lam, beta, None, 0, lms[V, 4][0], 0.0, lm_prebeam)
            exact = lambda h: (h[0],) + tuple(np.float64(x).tobytes() for x in h[1:4]) + (h[4],)      # noqa: E731
            assert [exact(h) for nb in got for h in nb] == [exact(h) for nb in want for h in nb]
            assert all(len(h) == 5 for nb in want for h in nb) and all(math.isfinite(h[5]) for nb in got for h in nb)
            assert sum(len(nb) for nb in got) > 0


@pytest.mark.parametrize("lm_prebeam", [True, False])
def test_a_finished_hypothesis_keeps_its_lm_while_it_waits(cases, lm_prebeam):
    """<eos> is likely at the first step and all but impossible afterwards: the hypothesis that ended at once keeps its slot,
    its scores and its LM sum - the </s> term after <s> - step after step, while the other slots go on growing."""
    c = R.SURVIVOR
    tables, lms = cases
    y, tab, lens, logp, lens_d, table = tables["survivor"]
    lm, plm = lms[c["V"], c["order"]]
    first = None
    for max_steps in (1, 2, 3, 4, 5):
        got = js.joint_beam_search(logp, lens_d, table_step_fn(table, c["beam"]), c["beam"], c["C"], c["V"] - 1, c["lam"], 0.0, max_steps,
                                   0, lm, c["lm_weight"], lm_prebeam)
        compare_search(got, R.yardstick(y, tab, lens, plm, c["beam"], c["C"], c["lam"], 0.0, max_steps, c["lm_weight"], lm_prebeam),
                       f"max_steps={max_steps}")
        for nb in got:
            assert [h[4] for h in nb] == [True, False, False] and nb[0][0] == [], nb
            assert all(len(h[0]) == max_steps for h in nb[1:]), nb
            assert nb[0][5] == lm.full_scores("", True, True)[0][0]
        first = first or [nb[0] for nb in got]
        assert [nb[0] for nb in got] == first, "the finished hypothesis changed while it waited"


@pytest.mark.parametrize("lm_prebeam", [True, False])
def test_one_step_with_the_lm_is_capturable(cases, lm_prebeam):
    """Score + prune of one step with the LM under torch.cuda.graph, replayed twice: the bits of the eager step."""
    tables, lms = cases
    y, tab, lens, logp, lens_d, table = tables["mid"]
    V = y.shape[2]
    lm = lms[V, 4][0]
    beam, C, lam, beta, w = 3, 5, 0.3, 0.5, 0.7
    fn = table_step_fn(table, beam)
    st = js.initial_state(logp, lens_d, beam, lam, 0, lm)
    for _ in range(2):
        st = js.search_step(logp, lens_d, st, fn(st.tokens, st.parents), beam, C, V - 1, lam, beta, 0, None, lm, w, lm_prebeam)
    att_logp = fn(st.tokens, st.parents)
    eager = js.search_step(logp, lens_d, st, att_logp, beam, C, V - 1, lam, beta, 0, None, lm, w, lm_prebeam)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = js.search_step(logp, lens_d, st, att_logp, beam, C, V - 1, lam, beta, 0, None, lm, w, lm_prebeam)
    for _ in range(2):
        for t in (out.tokens, out.total, out.att, out.ctc, out.lm):
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        alive = (eager.total > NEG).cpu()
        assert alive.any() and (eager.lm[alive.to(DEV)] != 0).all()
        assert torch.equal(out.tokens.cpu()[alive], eager.tokens.cpu()[alive])
        assert torch.equal(out.parents, eager.parents) and torch.equal(out.finished, eager.finished)
        for a, b in ((out.total, eager.total), (out.att, eager.att), (out.ctc, eager.ctc), (out.lm, eager.lm)):
            assert torch.equal(bits(a), bits(b))


# ---- end to end on the tiny Conformer --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_conformer(tmp_path_factory):
    from conftest import load_golden, load_golden_json
    from openeat_amd.models.asr_model import ASRModel
    g, meta = load_golden("f12_tiny_conformer"), load_golden_json("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    model.load_state_dict(g["sd"])
    lm = NgramLM(*R.make_lm(tmp_path_factory.mktemp("tiny_lm"), meta["V"], 3, 3))
    return model.to(DEV).eval(), g["in"]["feats"][:2].contiguous().to(DEV), g["in"]["flen"][:2].to(DEV), meta, lm


@pytest.mark.parametrize("lm_prebeam", [True, False])
def test_model_weight_zero_is_the_search_without_an_lm(tiny_conformer, lm_prebeam):
    model, feats, flen, meta, lm = tiny_conformer
    kw = dict(beam_size=3, ctc_weight=0.3, nbest=True, max_len=8)
    want = model.ctc_attention_beam_search(feats, flen, **kw)
    got = model.ctc_attention_beam_search(feats, flen, lm=lm, lm_weight=0.0, lm_prebeam=lm_prebeam, **kw)
    exact = lambda h: (h[0],) + tuple(np.float64(x).tobytes() for x in h[1:4])                            # noqa: E731
    assert [[exact(h) for h in nb] for nb in got] == [[exact(h) for h in nb] for nb in want]
    assert all(len(h) == 5 for nb in got for h in nb) and all(len(h) == 4 for nb in want for h in nb)
    assert model.ctc_attention_beam_search(feats, flen, beam_size=3, ctc_weight=0.3, max_len=8, lm=lm, lm_weight=0.0,
                                           lm_prebeam=lm_prebeam) == [nb[0][0] for nb in want]


@pytest.mark.parametrize("lm_prebeam", [True, False])
def test_model_hypotheses_carry_their_lm_score(tiny_conformer, lm_prebeam):
    """Every hypothesis' lm is ops.ngram_score of its tokens (bos = 1; eos = 1 when it is finished) and its total recomposes
    from att, ctc, length and lm.  The list does not say which hypotheses are finished: exactly one reading must fit each,
    finished ones first."""
    model, feats, flen, meta, lm = tiny_conformer
    lam, beta, w = 0.3, 0.25, 0.6
    res = model.ctc_attention_beam_search(feats, flen, beam_size=3, ctc_weight=lam, length_bonus=beta, nbest=True, max_len=8, lm=lm,
                                          lm_weight=w, lm_prebeam=lm_prebeam)
    assert len(res) == 2
    for nb in res:
        assert len(nb) == 3
        readings = []
        for tokens, total, att, ctc, m in nb:
            tk = torch.tensor([tokens + [0]], dtype=torch.int64, device=DEV)
            ln = torch.tensor([len(tokens)], dtype=torch.int64, device=DEV)
            fits = []
            for fin in (False, True):
                want = float(ops.ngram_score(lm, tk, ln, bos=True, eos=fin)[0])
                if abs(m - want) <= 1e-9 * max(1.0, abs(want)):
                    fits.append(fin)
            assert len(fits) == 1, (tokens, m)
            readings.append(fits[0])
            mix = (((1 - lam) * att + lam * ctc) + beta * len(tokens)) + w * m
            assert abs(total - mix) <= 1e-9 * max(1.0, abs(mix)), (tokens, total, mix)
        assert readings == sorted(readings, reverse=True), "finished hypotheses come first"
    best = model.ctc_attention_beam_search(feats, flen, beam_size=3, ctc_weight=lam, length_bonus=beta, max_len=8, lm=lm, lm_weight=w,
                                           lm_prebeam=lm_prebeam)
    assert best == [nb[0][0] for nb in res]


def test_model_refuses_an_lm_it_cannot_use(tiny_conformer, tmp_path):
    model, feats, flen, meta, lm = tiny_conformer
    small = NgramLM(*R.make_lm(tmp_path, meta["V"] - 1, 2, 1))
    for kw in (dict(lm=lm, lm_weight=float("nan")), dict(lm=lm, lm_weight=float("inf")), dict(lm="lm.arpa", lm_weight=0.5),
               dict(lm=small, lm_weight=0.5)):
        with pytest.raises(ValueError):
            model.ctc_attention_beam_search(feats, flen, beam_size=2, **kw)
    logp = torch.zeros(1, 2, meta["V"], device=DEV)
    for kw in (dict(lm=lm, lm_weight=float("nan")), dict(lm=object(), lm_weight=0.5)):
        with pytest.raises(ValueError):
            js.joint_beam_search(logp, None, lambda t, p: logp[:, 0], 1, 2, meta["V"] - 1, **kw)
