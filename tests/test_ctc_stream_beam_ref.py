"""CPU: the yardstick of the resumable prefix beam search (tests/ctc_stream_beam_ref.py) is pinned to the yardsticks that exist
(ctc_lm_beam_ref.search, ctc_bias_beam_ref.search), stops and resumes without a trace, commits what the live prefixes share,
and gives the emission frames a case worked by hand has."""
import numpy as np
import pytest

import ctc_bias_beam_ref as BR
import ctc_lm_beam_ref as R
import ctc_stream_beam_ref as S
import ngram_ref

GAP_FLOOR = 1e-8


def _case(tmp_path_factory, i):
    Bn, T, V, beam, sharp, order = R.CASES[i]
    logits, lens, path, t2c = R.make_case(tmp_path_factory.mktemp(f"stream{i}"), Bn, T, V, beam, sharp, order)
    tp, ti = BR.cpu_topk(logits, beam)
    return tp, ti, lens, R.PrefixLM(ngram_ref.RefLM(path), t2c), BR.case_graph(logits, lens, V, beam), beam


def _check_frames(nbest, frames, ti, T):
    """One emission frame per token, strictly increasing, inside the utterance, and the token is in that frame's top-k."""
    assert len(frames) == len(nbest)
    for h, fr in zip(nbest, frames):
        assert len(fr) == len(h[0]) and all(a < b for a, b in zip(fr, fr[1:])) and all(0 <= f < T for f in fr), (h, fr)
        assert all(tok in ti[f] for tok, f in zip(h[0], fr)), (h, fr)


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_one_chunk_is_the_existing_yardsticks(tmp_path_factory, i):
    tp, ti, lens, plm, graph, beam = _case(tmp_path_factory, i)
    for b in range(len(lens)):
        p, x = tp[b, : lens[b]], ti[b, : lens[b]]
        for lw, lb in BR.WEIGHTS:
            want, wgap = R.search(p, x, beam, plm, lw, lb, True)
            got, frames, gap, _ = S.search(p, x, beam, plm=plm, lm_weight=lw, length_bonus=lb)
            assert [h[:4] for h in got] == want and gap == wgap and all(h[4] == 0.0 for h in got)
            _check_frames(got, frames, x, lens[b])
            for use_lm in (True, False):
                for final in (True, False):
                    want, wgap = BR.search(p, x, beam, graph, plm if use_lm else None, lw, lb, True, final)
                    got, frames, gap, _ = S.search(p, x, beam, graph=graph, plm=plm if use_lm else None, lm_weight=lw, length_bonus=lb,
                                                   final=final)
                    assert got == want and gap == wgap, (b, lw, lb, use_lm, final)
                    _check_frames(got, frames, x, lens[b])
        want, _ = BR.search(p, x, beam, BR.make_graph([], 0.0))                 # the plain search
        got, frames, _, _ = S.search(p, x, beam)
        assert got == want


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_chunked_is_one_shot_and_the_stable_prefix_is_what_the_live_prefixes_share(tmp_path_factory, i):
    tp, ti, lens, plm, graph, beam = _case(tmp_path_factory, i)
    lw, lb = BR.WEIGHTS[1]
    grew = 0
    for b in range(len(lens)):
        p, x, T = tp[b, : lens[b]], ti[b, : lens[b]], int(lens[b])
        for kw in (dict(), dict(plm=plm, lm_weight=lw, length_bonus=lb), dict(graph=graph, length_bonus=lb),
                   dict(graph=graph, plm=plm, lm_weight=lw, length_bonus=lb, final=False)):
            want, _, wgap, _ = S.search(p, x, beam, **kw)
            for cuts in S.cut_sets(T)[1:]:
                edges = [0] + cuts + [T]
                st = S.Stream(beam, **kw)
                seen = []
                for a, e in zip(edges, edges[1:]):
                    st.push(p[a:e], x[a:e])
                    tokens, frames = st.stable()
                    assert tokens == st.lcp() and len(frames) == len(tokens)                  # all that is shared, nothing else
                    assert all(tokens[:len(s)] == s for s in seen[-1:])                       # it only grows
                    seen.append(tokens)
                    mid, mid_frames = st.nbest(False)
                    assert all(list(h[0][:len(tokens)]) == tokens for h in mid)
                    assert all(f[:len(frames)] == frames for f in mid_frames)
                    _check_frames(mid, mid_frames, x, T)
                got, frames = st.nbest(True)
                assert got == want and st.gap == wgap, (b, sorted(kw), cuts[:4])
                _check_frames(got, frames, x, T)
                for s in seen:                                                                # what was committed stayed true
                    assert all(list(h[0][:len(s)]) == s for h in got)
                grew += len(seen[-1]) > 0
    if beam > 1 and R.CASES[i][4] >= 1.0:
        assert grew > 0


def test_emission_frames_of_a_case_worked_by_hand():
    """Beam 2, two entries per frame, tokens 1 and 2.
    frame 0: blank -0.3, 2 -1.5          -> ()  -0.3 | (2) -1.5, made at frame 0
    frame 1: blank -0.2, 1 -1.0          -> ()  -0.5 | (1) -1.3, made at frame 1; (2) -1.7 and (2,1) -2.5 are cut: (2) drops out
    frame 2: 2 -0.5, 1 -0.6              -> () + 2 = (2) -1.0 is made AGAIN, at frame 2; () + 1 lands on the live (1), which also
                                            repeats: log_add(-1.1, -1.9) = -0.7289, and keeps frame 1; (1,2) -1.8 is cut and (),
                                            without a blank in the top-k, is gone
    frame 3: blank -0.4, 2 -1.2          -> (2) log_add(-1.4, -2.2) = -1.0289 | (1) -1.1289; (1,2) -1.9289 is cut
    So (2) carries frame 2, not 0, and (1) frame 1, not 2; nothing is ever shared by both live prefixes."""
    tp = [[-0.3, -1.5], [-0.2, -1.0], [-0.5, -0.6], [-0.4, -1.2]]
    ti = [[0, 2], [0, 1], [2, 1], [0, 2]]
    st = S.Stream(2)
    live = []
    for f in range(4):
        st.push(tp[f:f + 1], ti[f:f + 1])
        live.append([(p, st.frames[p]) for p, _ in st.cur])
    assert live == [[((), ()), ((2,), (0,))], [((), ()), ((1,), (1,))], [((1,), (1,)), ((2,), (2,))], [((2,), (2,)), ((1,), (1,))]]
    got, frames = st.nbest(True)
    assert [h[0] for h in got] == [(2,), (1,)] and frames == [[2], [1]] and st.stable() == ([], [])
    assert abs(got[0][1] - (-1.0288993340522223)) < 1e-15 and abs(got[1][1] - (-1.1288993340522224)) < 1e-15
    for cuts in ([], [1, 2, 3], [2], [1, 1, 3]):
        assert S.search(tp, ti, 2, cuts)[:2] == (got, frames)
    # beam 3 keeps (2) alive through frame 1: at frame 2 the extension () + 2 lands on it and it keeps frame 0
    got3, frames3, _, _ = S.search([r + [-9.0] for r in tp], [r + [3] for r in ti], 3)
    assert got3[0][0] == (2,) and frames3[0] == [0]


def test_the_long_case_commits_most_of_its_prefix():
    import torch
    T, V, beam, _, chunk = S.LONG
    lp = torch.log_softmax(S.long_case(), -1).numpy()[0]
    idx = np.argsort(-lp, axis=-1, kind="stable")[:, :beam]
    tp, ti = np.take_along_axis(lp, idx, -1), idx
    got, frames, gap, stables = S.search(tp, ti, beam, list(range(chunk, T, chunk)))
    assert gap >= GAP_FLOOR and len(got[0][0]) >= 150
    assert len(stables[-2][0]) > 100                                                          # before the last chunk already
    assert got == S.search(tp, ti, beam)[0]
    _check_frames(got, frames, ti, T)
