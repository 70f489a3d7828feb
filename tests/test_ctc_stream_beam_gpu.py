"""GPU: the resumable CTC prefix beam search (oe_ctc_prefix_beam_chunk, utils.stream_search.PrefixBeamStream).

Bounds.  Against the one-shot search (oe_ctc_prefix_beam) on the same device top-k: the SAME BITS in all six outputs, for every
variant and every way of cutting the frames - both run the same statements on the same numbers.  Against the Python yardstick
(tests/ctc_stream_beam_ref.py, pinned by tests/test_ctc_stream_beam_ref.py): the stable prefix and the emission frames are
integers and must be equal; the yardstick's neighbouring totals are 1e-8 apart or exactly equal on the top-k really used
(asserted, as in tests/test_ctc_bias_beam_gpu.py), so both sides keep the same prefixes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ctc_bias_beam_ref as BR  # noqa: E402
import ctc_lm_beam_ref as R  # noqa: E402
import ctc_stream_beam_ref as S  # noqa: E402
import ngram_ref  # noqa: E402
from openeat_amd.models.ngram_lm import NgramLM  # noqa: E402
from openeat_amd.utils.context_graph import ContextGraph  # noqa: E402
from openeat_amd.utils.stream_search import PrefixBeamStream  # noqa: E402

DEV = "cuda"
GAP_FLOOR = 1e-8
VARIANTS = ("plain", "lm", "ctx", "lmctx")
SCORES = {"plain": ("total",), "lm": ("total", "ctc", "lm"), "ctx": ("total", "ctc", "bias"), "lmctx": ("total", "ctc", "lm", "bias")}


def _bits(x):
    return x.contiguous().view(torch.int64)


def _used(pre, plen):
    return pre[torch.arange(pre.shape[2], device=pre.device).view(1, 1, -1) < plen.unsqueeze(2)]


def _schedules(L):
    """Per schedule the list of chunks, a chunk the frames each utterance gets -> {name: [[frames of b]]}.  `ragged` gives
    utterance b chunks of 7 + 3 b frames, so they end in different chunks, and ends with a chunk without any frame."""
    def by(sizes):
        rem, out = list(L), []
        for k in range(10 ** 6):
            row = [min(r, sizes(k, b)) for b, r in enumerate(rem)]
            rem = [r - x for r, x in zip(rem, row)]
            out.append(row)
            if not any(rem):
                return out
    return {"one": [list(L)],
            "each": by(lambda k, b: 1),
            "1-0-5-rest": by(lambda k, b: (1, 0, 5)[k] if k < 3 else 10 ** 9),
            "ragged": by(lambda k, b: 7 + 3 * b) + [[0] * len(L)]}


def _chunks(top_p, top_i, schedule):
    """-> [(top_p (B, Tk, beam), top_i, lens (B) int32 on the device)], Tk >= 1."""
    B, _, beam = top_p.shape
    off = [0] * B
    for row in schedule:
        Tk = max(max(row), 1)
        cp = torch.zeros(B, Tk, beam, device=DEV)
        ci = torch.zeros(B, Tk, beam, dtype=torch.int64, device=DEV)
        for b, n in enumerate(row):
            cp[b, :n] = top_p[b, off[b]:off[b] + n]
            ci[b, :n] = top_i[b, off[b]:off[b] + n]
            off[b] += n
        yield cp, ci, torch.tensor(row, dtype=torch.int32, device=DEV)


def _one_shot(variant, top_p, top_i, dlens, beam, lm, graph, lw, lb, final=True):
    from openeat_amd import hip
    if variant == "plain":
        pre, plen, total, bad = hip.ctc_prefix_beam_device(top_p, top_i, dlens, beam, raw=True)
        out = dict(total=total)
    elif variant == "lm":
        pre, plen, total, ctc, lms, bad = hip.ctc_prefix_beam_lm_device(top_p, top_i, dlens, beam, lm, lw, lb, True, raw=True)
        out = dict(total=total, ctc=ctc, lm=lms)
    else:
        pre, plen, total, ctc, lms, bias, bad = hip.ctc_prefix_beam_ctx_device(top_p, top_i, dlens, beam, graph, lm if variant == "lmctx" else None,
                                                                               lw, lb, True, final, raw=True)
        out = dict(total=total, ctc=ctc, lm=lms, bias=bias)
    assert int(bad[0]) == 0
    return dict(out, prefixes=pre, plen=plen)


def _stream(variant, B, beam, max_len, lm, graph, lw, lb, final=True):
    if variant == "plain":
        return PrefixBeamStream(B, beam, max_len, DEV)
    return PrefixBeamStream(B, beam, max_len, DEV, lm if variant in ("lm", "lmctx") else None, graph if variant in ("ctx", "lmctx") else None,
                            lw, lb, True, final)


def _same_bits(got, want, variant, where):
    assert torch.equal(got["plen"], want["plen"]), where
    assert torch.equal(_used(got["prefixes"], got["plen"]), _used(want["prefixes"], want["plen"])), where
    for k in SCORES[variant]:
        assert torch.equal(_bits(got[k]), _bits(want[k])), (where, k)


def _case(tmp_path, B, T, V, beam, sharp, order):
    from openeat_amd import ops
    logits, lens, path, t2c = R.make_case(tmp_path, B, T, V, beam, sharp, order)
    ref_graph = BR.case_graph(logits, lens, V, beam)
    top_p, top_i = ops.topk_rows(logits.to(DEV), beam, log_softmax=True)
    return (top_p, top_i, lens, NgramLM(path, t2c), ContextGraph(ref_graph[0], float(ref_graph[2]), ref_graph[1]),
            R.PrefixLM(ngram_ref.RefLM(path), t2c), ref_graph)


@pytest.mark.parametrize("B,T,V,beam,sharp,order", R.CASES)
def test_chunked_is_the_one_shot_search_bit_for_bit(tmp_path, B, T, V, beam, sharp, order):
    top_p, top_i, lens, lm, graph, _, _ = _case(tmp_path, B, T, V, beam, sharp, order)
    dlens = lens.to(DEV)
    schedules = _schedules(lens.tolist())
    ends = {max(k for k, row in enumerate(schedules["ragged"]) if row[b]) for b in range(B) if lens[b]}
    assert len(ends) > 1                                                    # the utterances end in different chunks
    for variant in VARIANTS:
        for lw, lb in BR.WEIGHTS:
            final = lb == 0.0
            want = _one_shot(variant, top_p, top_i, dlens, beam, lm, graph, lw, lb, final)
            for name, schedule in schedules.items():
                st = _stream(variant, B, beam, T, lm, graph, lw, lb, final)
                for k, chunk in enumerate(_chunks(top_p, top_i, schedule)):
                    got = st.push(*chunk, last=k == len(schedule) - 1, emit=k % 2 == 0, raw=True)
                torch.cuda.synchronize()
                assert int(got["status"][0]) == 0
                _same_bits(got, want, variant, (variant, lw, lb, name))
            if variant == "plain":
                break


def test_a_single_chunk_without_any_state(tmp_path):
    """state_in NULL, state_out NULL, last: the one-shot search through the other entry point."""
    from openeat_amd import hip
    B, T, V, beam, sharp, order = R.CASES[0]
    top_p, top_i, lens, lm, graph, _, _ = _case(tmp_path, B, T, V, beam, sharp, order)
    dlens = lens.to(DEV)
    lw, lb = BR.WEIGHTS[1]
    want = _one_shot("lmctx", top_p, top_i, dlens, beam, lm, graph, lw, lb)
    ws = torch.zeros(hip.lib().oe_ctc_prefix_beam_workspace_bytes(B, T, beam) // 4, dtype=torch.int32, device=DEV)
    pre = torch.zeros(B, beam, T, dtype=torch.int32, device=DEV)
    frm = torch.full((B, beam, T), -1, dtype=torch.int32, device=DEV)
    plen = torch.zeros(B, beam, dtype=torch.int32, device=DEV)
    sc = [torch.zeros(B, beam, dtype=torch.float64, device=DEV) for _ in range(4)]
    stable = [torch.zeros(B, T, dtype=torch.int32, device=DEV), torch.zeros(B, T, dtype=torch.int32, device=DEV),
              torch.zeros(B, dtype=torch.int32, device=DEV)]
    a = hip.prefix_beam_args(top_p, top_i, dlens, beam, T, ws, pre, plen, *sc, lm=hip.ngram_model(lm, DEV), ctx=hip.context_graph(graph, DEV),
                             lm_weight=lw, length_bonus=lb, eos=True, final=True)
    hip.prefix_beam_chunk(a, None, None, *stable, frm, last=True, emit=False)
    torch.cuda.synchronize()
    assert int(ws[-1]) == 0
    _same_bits(dict(prefixes=pre, plen=plen, total=sc[0], ctc=sc[1], lm=sc[2], bias=sc[3]), want, "lmctx", "no state")
    used = _used(frm, plen).cpu().numpy()
    assert (used >= 0).all() and (used < T).all()


@pytest.mark.parametrize("B,T,V,beam,sharp,order", R.CASES)
def test_frames_and_stable_prefix_equal_the_yardstick(tmp_path, B, T, V, beam, sharp, order):
    top_p, top_i, lens, lm, graph, plm, ref_graph = _case(tmp_path, B, T, V, beam, sharp, order)
    hp, hi = top_p.cpu().numpy(), top_i.cpu().numpy()
    L = lens.tolist()
    schedules = _schedules(L)
    lw, lb = BR.WEIGHTS[1]
    kws = {"plain": dict(), "lm": dict(plm=plm, lm_weight=lw, length_bonus=lb), "ctx": dict(graph=ref_graph, length_bonus=lb),
           "lmctx": dict(graph=ref_graph, plm=plm, lm_weight=lw, length_bonus=lb)}
    grew = 0
    for variant in VARIANTS:
        for name in ("1-0-5-rest", "ragged"):
            schedule = schedules[name]
            st = _stream(variant, B, beam, T, lm, graph, lw, lb)
            refs = [S.Stream(beam, **kws[variant]) for _ in range(B)]
            off = [0] * B
            for k, chunk in enumerate(_chunks(top_p, top_i, schedule)):
                last = k == len(schedule) - 1
                got = st.push(*chunk, last=last)
                for b in range(B):
                    n = schedule[k][b]
                    refs[b].push(hp[b, off[b]:off[b] + n], hi[b, off[b]:off[b] + n])
                    off[b] += n
                    want, frames = refs[b].nbest(last)
                    where = (variant, name, k, b)
                    assert got[b]["stable"] == refs[b].stable(), where
                    assert [h[0] for h in got[b]["nbest"]] == [h[0] for h in want], where
                    assert got[b]["frames"] == frames, where
                    assert all(abs(g[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])) for g, w in zip(got[b]["nbest"], want)), where
                    grew += len(got[b]["stable"][0]) > 0 and not last
            for b in range(B):
                assert refs[b].gap >= GAP_FLOOR, (variant, name, b, refs[b].gap)       # the case is decidable on this top-k
    if beam > 1 and sharp >= 1.0:
        assert grew > 0


def test_a_long_prefix_is_committed_as_it_grows():
    from openeat_amd import ops
    T, V, beam, _, chunk = S.LONG
    top_p, top_i = ops.topk_rows(S.long_case().to(DEV), beam, log_softmax=True)
    ref = S.Stream(beam)
    hp, hi = top_p.cpu().numpy()[0], top_i.cpu().numpy()[0]
    want = _one_shot("plain", top_p, top_i, None, beam, None, None, 0.0, 0.0)
    st = PrefixBeamStream(1, beam, T, DEV)
    longest = 0
    for a in range(0, T, chunk):
        last = a + chunk >= T
        got = st.push(top_p[:, a:a + chunk], top_i[:, a:a + chunk], last=last, emit=last, raw=True)
        ref.push(hp[a:a + chunk], hi[a:a + chunk])
        stable = st.stable()[0]
        assert stable == ref.stable()
        if not last:
            longest = len(stable[0])
    assert ref.gap >= GAP_FLOOR
    assert longest > 100
    assert int(got["status"][0]) == 0 and int(got["plen"][0, 0]) >= 150
    _same_bits(got, want, "plain", "long")
    nbest, frames = ref.nbest(True)
    n = int(got["plen"][0, 0])
    assert got["prefixes"][0, 0, :n].tolist() == list(nbest[0][0]) and got["frames"][0, 0, :n].tolist() == frames[0]


def test_status_words(tmp_path):
    from openeat_amd import hip
    B, T, V, beam, sharp, order = R.CASES[0]
    top_p, top_i, lens, lm, graph, _, _ = _case(tmp_path, B, T, V, beam, sharp, order)
    dlens = lens.to(DEV)
    # max_len too small
    st = PrefixBeamStream(B, beam, 2, DEV)
    got = st.push(top_p, top_i, dlens, last=True, raw=True)
    torch.cuda.synchronize()
    assert int(got["status"][0]) == 1
    with pytest.raises(RuntimeError, match="exceeded max_len"):
        PrefixBeamStream(B, beam, 2, DEV).push(top_p, top_i, dlens, last=True)
    # a state of the plain search fed to the LM-fused one: status 2, nothing written
    plain = PrefixBeamStream(B, beam, T, DEV)
    plain.push(top_p[:, :20], top_i[:, :20], raw=True)
    fused = PrefixBeamStream(B, beam, T, DEV, lm, None, 0.5, 0.0)
    fused._cur = plain._cur
    for t in (fused.prefixes, fused.frames, fused.plen, fused.stable_prefix, fused.stable_frame, fused.stable_len):
        t.fill_(7)
    for t in (fused.total, fused.ctc, fused.lms):
        t.fill_(7.0)
    fused._states[0].fill_(7)
    got = fused.push(top_p[:, 20:], top_i[:, 20:], last=True, raw=True)
    torch.cuda.synchronize()
    assert int(got["status"][0]) == 2
    for t in (fused.prefixes, fused.frames, fused.plen, fused.stable_prefix, fused.stable_frame, fused.stable_len, fused._states[0]):
        assert bool((t == 7).all())
    for t in (fused.total, fused.ctc, fused.lms):
        assert bool((t == 7.0).all())
    fused.reset()
    fused._cur = plain._cur
    with pytest.raises(RuntimeError, match="another search"):
        fused.push(top_p[:, 20:], top_i[:, 20:], last=True)


def test_bad_arguments_are_reported_not_launched():
    from openeat_amd import hip
    B, T, beam = 2, 6, 4
    top_p = torch.zeros(B, T, beam, device=DEV)
    top_i = torch.zeros(B, T, beam, dtype=torch.int64, device=DEV)
    ws = torch.zeros(hip.lib().oe_ctc_prefix_beam_workspace_bytes(B, T, beam) // 4, dtype=torch.int32, device=DEV)
    pre = torch.zeros(B, beam, T, dtype=torch.int32, device=DEV)
    plen = torch.zeros(B, beam, dtype=torch.int32, device=DEV)
    score = torch.zeros(B, beam, dtype=torch.float64, device=DEV)
    n = hip.lib().oe_ctc_prefix_beam_state_bytes(B, beam, T)
    assert n > 0 and hip.lib().oe_ctc_prefix_beam_state_bytes(B, 17, T) == 0
    s0, s1 = (torch.zeros(n, dtype=torch.uint8, device=DEV) for _ in range(2))
    stable = [torch.zeros(B, T, dtype=torch.int32, device=DEV), torch.zeros(B, T, dtype=torch.int32, device=DEV),
              torch.zeros(B, dtype=torch.int32, device=DEV)]
    a = hip.prefix_beam_args(top_p, top_i, None, beam, T, ws, pre, plen, score)
    bad_beam = hip.prefix_beam_args(top_p, top_i, None, 17, T, ws, pre, plen, score)
    no_out = hip.prefix_beam_args(top_p, top_i, None, beam, T, ws, pre, plen, None)
    weights = hip.prefix_beam_args(top_p, top_i, None, beam, T, ws, pre, plen, score, lm_weight=0.5)
    for args, kw, message in (((a, None, None, *stable), dict(last=False), "state_out"),
                              ((a, s0, s0, *stable), dict(last=True), "alias"),
                              ((a, None, s1, None, stable[1], stable[2]), {}, "null pointer"),
                              ((a, None, s1, stable[0], None, stable[2]), {}, "null pointer"),
                              ((a, None, s1, stable[0], stable[1], None), {}, "null pointer"),
                              ((bad_beam, None, s1, *stable), {}, "beam must be 1..16"),
                              ((no_out, None, s1, *stable), {}, "null pointer"),
                              ((weights, None, s1, *stable), {}, "plain search")):
        with pytest.raises(RuntimeError, match=message):
            hip.prefix_beam_chunk(*args, **kw)
    c = hip.PrefixBeamChunk()
    assert hip.lib().oe_ctc_prefix_beam_chunk(ctypes.byref(c), None) != 0 and b"search" in hip.lib().oe_last_error()
    assert hip.lib().oe_ctc_prefix_beam_chunk(None, None) != 0 and b"null pointer" in hip.lib().oe_last_error()
    torch.cuda.synchronize()
    assert int(plen.abs().sum()) == 0 and float(score.abs().sum()) == 0.0 and int(s1.sum()) == 0 and int(stable[2].sum()) == 0      # nothing ran


def test_one_captured_chunk_replayed_twice_gives_the_eager_bits(tmp_path):
    B, T, V, beam, sharp, order = R.CASES[0]
    top_p, top_i, lens, lm, graph, _, _ = _case(tmp_path, B, T, V, beam, sharp, order)
    lw, lb = BR.WEIGHTS[1]
    half = T // 2
    first = (top_p[:, :half].contiguous(), top_i[:, :half].contiguous(), lens.clamp(max=half).to(DEV))
    second = (top_p[:, half:].contiguous(), top_i[:, half:].contiguous(), (lens - half).clamp(min=0).to(DEV))
    keys = ("prefixes", "frames", "plen", "total", "ctc", "lm", "bias", "stable_prefix", "stable_frame", "stable_len")
    st = _stream("lmctx", B, beam, T, lm, graph, lw, lb)
    st.push(*first, raw=True)
    stable_len = st.stable_len.clone()
    eager = {k: v.clone() for k, v in st.push(*second, last=True, raw=True).items()}
    torch.cuda.synchronize()
    st.reset()
    st.push(*first, raw=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = st.push(*second, last=True, raw=True)
    for _ in range(2):
        for k in keys[:7]:
            out[k].fill_(7)
        st.stable_len.copy_(stable_len)
        g.replay()
        torch.cuda.synchronize()
        assert int(out["status"][0]) == 0
        _same_bits(out, eager, "lmctx", "replay")
        assert torch.equal(out["stable_len"], eager["stable_len"])
        assert torch.equal(_used(out["frames"], out["plen"]), _used(eager["frames"], eager["plen"]))
        n = out["stable_len"]
        keep = torch.arange(T, device=DEV).view(1, -1) < n.view(-1, 1)
        assert torch.equal(out["stable_prefix"][keep], eager["stable_prefix"][keep])
        assert torch.equal(out["stable_frame"][keep], eager["stable_frame"][keep])
