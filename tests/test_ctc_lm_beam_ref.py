"""CPU: the yardstick of the LM-fused prefix beam search (tests/ctc_lm_beam_ref.py) is held to what is already pinned - with
zero weights it is the host recursion oe_ctc_prefix_beam_host_batch, its LM column is RefLM.score - and the cases the GPU
test runs are shown to be decidable (no two neighbouring totals closer than 1e-8 relative, unless exactly equal) and not
vacuous (the fused search finds 1-best hypotheses the plain n-best does not contain)."""
import numpy as np
import pytest
import torch

import ctc_lm_beam_ref as R
import ngram_ref

GAP_FLOOR = 1e-8          # ten times the 1e-9 the device-beam tests allow a score to differ by


def topk_host(logits, beam):
    """Per frame the `beam` largest log-probabilities, ties to the lowest index (as ops.topk_rows orders them)."""
    lp = torch.log_softmax(logits, -1).numpy()
    idx = np.argsort(-lp, axis=-1, kind="stable")[..., :beam]
    return np.take_along_axis(lp, idx, -1), idx.astype(np.int64)


_cache = {}


def _case(tmp_path_factory, i):
    """(top_p, top_i, lens, RefLM, token2char, {(weights, eos): per utterance (n-best, gap)}) of random case i, made once."""
    if i not in _cache:
        B, T, V, beam, sharp, order = R.CASES[i]
        logits, lens, path, t2c = R.make_case(tmp_path_factory.mktemp(f"case{i}"), B, T, V, beam, sharp, order)
        ref = ngram_ref.RefLM(path)
        assert ref.order == order
        top_p, top_i = topk_host(logits, beam)
        plm = R.PrefixLM(ref, t2c)
        runs = {}
        for w in R.WEIGHTS:
            for eos in (True, False):
                runs[(w, eos)] = [R.search(top_p[b, : lens[b]], top_i[b, : lens[b]], beam, plm, w[0], w[1], eos) for b in range(B)]
        _cache[i] = (top_p, top_i, lens, ref, t2c, runs)
    return _cache[i]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_zero_weights_give_the_host_recursion(tmp_path_factory, i):
    from openeat_amd import hip
    top_p, top_i, lens, _, _, runs = _case(tmp_path_factory, i)
    beam = R.CASES[i][3]
    want = hip.ctc_prefix_beam_host_batch(torch.from_numpy(top_p), torch.from_numpy(top_i), lens.tolist(), beam)
    for eos in (True, False):
        for b, (got, _) in enumerate(runs[((0.0, 0.0), eos)]):
            assert [h[0] for h in got] == [p for p, _ in want[b]], (b, eos)
            for h, (_, s) in zip(got, want[b]):
                assert abs(h[1] - s) <= 1e-12 * max(1.0, abs(s)) and h[1] == h[2], (b, h, s)
    assert len(runs[((0.0, 0.0), True)][1][0]) == 1 or i != 0          # the zero-frame utterance: the one empty prefix


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_lm_column_is_the_sentence_score(tmp_path_factory, i):
    _, _, _, ref, t2c, runs = _case(tmp_path_factory, i)
    for (w, eos), per_utt in runs.items():
        for got, _ in per_utt:
            for prefix, total, ctc, lm in got:
                want, n, S = ref.score(" ".join(t2c[t] for t in prefix), bos=True, eos=eos)
                assert abs(lm - want) <= 2.0 ** -52 * n * S, (prefix, lm, want)
                assert total == ctc + w[0] * lm + w[1] * len(prefix)


def test_every_gpu_case_keeps_its_neighbours_apart(tmp_path_factory):
    worst = np.inf
    for i in range(len(R.CASES)):
        runs = _case(tmp_path_factory, i)[5]
        for key, per_utt in runs.items():
            g = min(gap for _, gap in per_utt)
            print(f"case {R.CASES[i]} weights {key[0]} eos {key[1]}: smallest non-zero gap {g:.3g}")
            assert g >= GAP_FLOOR, (R.CASES[i], key, g)
            worst = min(worst, g)
    print(f"smallest gap of all: {worst:.3g}")


# The cases in which the search has something to decide: more than one prefix survives a frame (beam > 1) and the frames
# differ (sharp > 0).  They are the four whose figures the feature was motivated with.  The other two cannot show the property
# whatever the search does, and are measured and printed below instead: at beam 1 a frame offers ONE token, so the only
# choice an LM could change - stay or extend on a token repeated after a blank - has to occur by chance, and in these
# 4 x 33 frames over 40 tokens it does not; on uniform frames with a 1-gram model every n-best list is the same handful of
# shortest prefixes at either weight.
CHOICE_CASES = [i for i, c in enumerate(R.CASES) if c[3] > 1 and c[4] > 0.0]


def _outside(runs):
    plain, fused = runs[((0.0, 0.0), True)], runs[((0.5, 0.0), True)]
    return sum(f[0][0][0] not in {h[0] for h in p[0]} for f, p in zip(fused, plain)), len(plain)


@pytest.mark.parametrize("i", CHOICE_CASES)
def test_fusion_finds_what_the_plain_nbest_lost(tmp_path_factory, i):
    """At lm_weight 0.5 at least one utterance's fused 1-best is absent from the weight-0 n-best: rescoring that n-best could
    not have found it.  Measured: 4 of 5 (the fifth utterance has no frames), 8 of 8, 3 of 3, 2 of 2."""
    outside, n = _outside(_case(tmp_path_factory, i)[5])
    print(f"case {R.CASES[i]}: fused 1-best outside the plain n-best for {outside} of {n} utterances")
    assert outside >= 1


def test_cases_without_a_choice_are_the_expected_two(tmp_path_factory):
    """The cases left out above are exactly beam 1 and the uniform frames; what they give is printed (measured: 0 of 4, 0 of 6)."""
    rest = [i for i in range(len(R.CASES)) if i not in CHOICE_CASES]
    assert [R.CASES[i][:5] for i in rest] == [(4, 33, 40, 1, 1.0), (6, 25, 5, 5, 0.0)] and len(CHOICE_CASES) == 4
    for i in rest:
        outside, n = _outside(_case(tmp_path_factory, i)[5])
        print(f"case {R.CASES[i]}: fused 1-best outside the plain n-best for {outside} of {n} utterances")


def test_tie_case_has_exact_ties_at_the_top(tmp_path):
    """Uniform frames, every word at log10 p = -1: whole groups of prefixes share a total exactly, and the order inside a
    group is insertion order - the case the device has to reproduce."""
    logits, lens, path, t2c, beam = R.tie_case(tmp_path)
    plm = R.PrefixLM(ngram_ref.RefLM(path), t2c)
    top_p, top_i = topk_host(logits, beam)
    for w in ((0.5, 0.0), (0.5, 1.0)):
        for b in range(logits.shape[0]):
            got, gap = R.search(top_p[b, : lens[b]], top_i[b, : lens[b]], beam, plm, w[0], w[1], True)
            totals = [h[1] for h in got]
            print(f"weights {w} utterance {b}: totals {totals}")
            assert gap >= GAP_FLOOR
            if b == 0:                                                  # all 25 frames: three prefixes share the best total
                assert totals[0] == totals[1] == totals[2], (w, totals)
