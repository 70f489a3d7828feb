"""CPU: host-side logic of the product (no kernels launched): helper tables against the
reference's golden vectors, checkpoint layout, scheduler, and the no-CPU-fallback rule."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, load_golden_json
from openeat_amd.models.asr_model import ASRModel
from openeat_amd.utils import common as C
from openeat_amd.utils import mask as M
from openeat_amd.utils.checkpoint import load_checkpoint, load_trained_modules, save_checkpoint
from openeat_amd.utils.cmvn import load_cmvn
from openeat_amd.utils.scheduler import WarmupLR


def test_helper_tables_match_reference_f10():
    j = load_golden_json("f10_helpers")
    ys = torch.tensor(j["ys"], dtype=torch.int32)
    ys_in, ys_out = C.add_sos_eos(ys, 10, 11, -1)
    assert ys_in.tolist() == j["ys_in"] and ys_out.tolist() == j["ys_out"]
    assert ys_in.dtype == torch.long and ys_out.dtype == torch.long
    assert C.reverse_pad_list(ys, torch.tensor(j["lens"]), -1.0).tolist() == j["rev"]
    assert M.make_pad_mask(torch.tensor([5, 3, 2])).int().tolist() == j["pad_mask"]
    assert M.make_pad_mask(torch.tensor([5, 3, 2]), 8).int().tolist() == j["pad_mask8"]
    assert M.subsequent_mask(5).int().tolist() == j["subsequent"]
    assert [C.remove_duplicates_and_blank(p) for p in j["paths"]] == j["collapsed"]
    la = [C.log_add([-1.0, -2.5, -float("inf")]), C.log_add([-float("inf")] * 2), C.log_add([0.3])]
    for a, b in zip(la, j["log_add"]):
        b = -float("inf") if b == "-inf" else b
        assert a == b or abs(a - b) < 1e-12


def test_add_sos_eos_static_shapes_and_interior_padding():
    ys = torch.tensor([[3, 4, 5], [6, -1, -1]], dtype=torch.int32)
    C.STATIC_SHAPES = True
    try:
        a, b = C.add_sos_eos(ys, 9, 9, -1)
        r = C.reverse_pad_list(ys, torch.tensor([3, 1]), -1)
    finally:
        C.STATIC_SHAPES = False
    assert a.tolist() == [[9, 3, 4, 5], [9, 6, 9, 9]] and b.tolist() == [[3, 4, 5, 9], [6, 9, -1, -1]]
    assert r.tolist() == [[5, 4, 3], [6, -1, -1]]
    # the reference drops ignore_id wherever it sits (common.py:126)
    a, b = C.add_sos_eos(torch.tensor([[-1, 7, 8]]), 9, 9, -1)
    assert a.tolist() == [[9, 7, 8]] and b.tolist() == [[7, 8, 9]]


def test_finished_beam_masks():
    score = torch.zeros(4, 3)
    flag = torch.tensor([[True], [False], [True], [False]])
    out = M.mask_finished_scores(score.clone() + 1.5, flag)
    assert out[0].tolist() == [0.0, -float("inf"), -float("inf")] and out[1].tolist() == [1.5] * 3
    pred = M.mask_finished_preds(torch.arange(12).view(4, 3), flag, 99)
    assert pred[0].tolist() == [99] * 3 and pred[1].tolist() == [3, 4, 5]


def test_state_dict_layout_matches_reference_checkpoint():
    meta = load_golden_json("f12_tiny_conformer")
    g = load_golden("f12_tiny_conformer")
    model = ASRModel(80, meta["V"], **meta["kwargs"])
    own = model.state_dict()
    assert list(own.keys()) == list(g["sd"].keys())            # same keys, same order as the reference
    for k, v in g["sd"].items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    model.load_state_dict(g["sd"])                              # a reference checkpoint loads strictly
    meta11 = load_golden_json("f11_config1_transformer")
    m11 = ASRModel(80, meta11["V"], **meta11["kwargs"])
    assert [[k, list(p.shape)] for k, p in m11.named_parameters()] == meta11["param_order"]


def test_unknown_config_key_raises_like_the_reference():
    with pytest.raises(TypeError):
        ASRModel(80, 50, not_a_key=1)


def test_checkpoint_roundtrip(tmp_path):
    m = ASRModel(80, 30, encoder_num_blocks=1, decoder_num_blocks=1, d_model=16, attention_heads=4, linear_units=32)
    path = str(tmp_path / "3.pt")
    save_checkpoint(m, path, {"epoch": 3, "lr": 0.001, "step": 77})
    assert os.path.exists(str(tmp_path / "3.yaml"))
    sd = torch.load(path)
    assert list(sd.keys()) == list(m.state_dict().keys())       # flat state_dict, no wrapper key
    m2 = ASRModel(80, 30, encoder_num_blocks=1, decoder_num_blocks=1, d_model=16, attention_heads=4, linear_units=32)
    info = load_checkpoint(m2, path)
    assert info == {"epoch": 3, "lr": 0.001, "step": 77}
    for a, b in zip(m.state_dict().values(), m2.state_dict().values()):
        assert torch.equal(a, b)
    m3 = ASRModel(80, 30, encoder_num_blocks=1, decoder_num_blocks=1, d_model=16, attention_heads=4, linear_units=32)
    before = m3.decoder.left_decoder.output_layer.weight.clone()
    load_trained_modules(m3, path, ["encoder.", "ctc."])
    assert torch.equal(m3.ctc.ctc_lo.weight, m.ctc.ctc_lo.weight)
    assert torch.equal(m3.decoder.left_decoder.output_layer.weight, before)


def test_warmup_lr_and_cmvn_match_reference_f13():
    g = load_golden("f13_misc")
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-3)
    sch = WarmupLR(opt, warmup_steps=25)
    lrs = []
    for _ in range(60):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    np.testing.assert_allclose(np.array(lrs), g["out"]["lrs"].numpy(), rtol=1e-12)
    mean, istd = load_cmvn(os.path.join(GOLDEN, "f13_cmvn_stats.json"), True)
    np.testing.assert_allclose(mean, g["out"]["cmvn_mean"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(istd, g["out"]["cmvn_istd"].numpy(), rtol=1e-12)


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently computing on the host."""
    from openeat_amd import ops
    with pytest.raises(TypeError, match="no CPU fallback"):
        ops.layer_norm(torch.randn(4, 32), torch.ones(32), torch.zeros(32), 1e-5)
    m = ASRModel(80, 30, encoder_num_blocks=1, decoder_num_blocks=1, d_model=16, attention_heads=4, linear_units=32)
    with pytest.raises(TypeError, match="no CPU fallback"):
        m(torch.randn(2, 40, 80), torch.tensor([40, 30]), torch.randint(1, 29, (2, 4), dtype=torch.int32),
          torch.tensor([4, 3], dtype=torch.int32))


def test_product_never_imports_the_oracle():
    import subprocess
    import sys
    code = ("import sys; import openeat_amd.models.asr_model, openeat_amd.ops; "
            "bad=[m for m in sys.modules if m=='oracle' or m.startswith('oracle.')]; assert not bad, bad")
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(GOLDEN) + "/..")


def test_native_prefix_beam_search_host_code():
    """oe_ctc_prefix_beam_host is host code: checked on the CPU against the oracle's restatement of
    asr_model.py:359-396 (incl. exact ties, which exercise the stable pruning order)."""
    from openeat_amd import hip
    from oracle import asr as O
    torch.manual_seed(40)
    for trial in range(12):
        T, V, beam = 5 + 7 * trial, 12 + trial, 1 + trial % 6
        logits = torch.randn(T, V) * (1 + trial % 3)
        if trial % 2 == 0:
            logits = (logits * 2).round() / 2
        logp = torch.log_softmax(logits, -1)
        tp, ti = logp.topk(beam, dim=1)
        got = hip.ctc_prefix_beam_host(tp, ti, beam)
        want = O.prefix_beam_from_logp(logp, beam)
        assert [p for p, _ in got] == [p for p, _ in want]
        for (_, a), (_, b) in zip(got, want):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b))


def test_native_prefix_beam_search_batch_matches_per_utterance_and_oracle():
    """The threaded batch entry (ragged lengths, long emitting utterances) gives, per utterance, exactly what the
    single-utterance entry and the oracle give."""
    from openeat_amd import hip
    from oracle import asr as O
    torch.manual_seed(41)
    B, T, V, beam = 9, 60, 30, 5
    logits = torch.randn(B, T, V) * 3
    logits[:, :, 0] -= 2.0                      # few blanks: prefixes grow to tens of tokens
    logits[4] = (logits[4] * 2).round() / 2     # exact ties
    logp = torch.log_softmax(logits, -1)
    lens = [60, 1, 37, 60, 59, 0, 12, 60, 45]
    tp, ti = logp.topk(beam, dim=2)
    got = hip.ctc_prefix_beam_host_batch(tp, ti, lens, beam, n_threads=4)
    assert len(got) == B
    for b in range(B):
        one = hip.ctc_prefix_beam_host(tp[b, : lens[b]].contiguous(), ti[b, : lens[b]].contiguous(), beam)
        assert got[b] == one
        want = O.prefix_beam_from_logp(logp[b, : lens[b]], beam)
        assert [p for p, _ in got[b]] == [p for p, _ in want]
        for (_, a), (_, w) in zip(got[b], want):
            assert abs(a - w) <= 1e-12 * max(1.0, abs(w))
    assert max(len(p) for p, _ in got[0]) > 20


def test_public_method_surface_matches_reference_f22():
    """Every public method of the reference's hot-path classes (tests/golden/f22_api_signatures.json, written by
    make_fixtures.py from inspect.signature of the reference) exists here under the same import path, takes the
    reference's parameters in the reference's order with the reference's defaults; parameters added here (fused
    residual / dropout hooks) come after them and are optional."""
    import importlib
    import inspect
    ref = load_golden_json("f22_api_signatures")
    assert len(ref) >= 20
    problems = []
    for qual, methods in ref.items():
        mod, cls = qual.rsplit(".", 1)
        ours = getattr(importlib.import_module(mod), cls)                  # `openeat.*` is the alias package of the boundary
        for name, params in methods.items():
            fn = getattr(ours, name, None)
            if fn is None:
                problems.append(f"{qual}.{name}: missing")
                continue
            mine = list(inspect.signature(fn).parameters.items())
            if any(p.kind is inspect.Parameter.VAR_POSITIONAL or p.kind is inspect.Parameter.VAR_KEYWORD for _, p in mine):
                continue                                                   # **kwargs pass-through keeps the call contract
            for i, (pn, default) in enumerate(params):
                if i >= len(mine) or mine[i][0] != pn:
                    problems.append(f"{qual}.{name}: parameter {i} is {mine[i][0] if i < len(mine) else None!r}, reference has {pn!r}")
                    break
                d = mine[i][1].default
                got = None if d is inspect.Parameter.empty else repr(d)
                if got != default:
                    problems.append(f"{qual}.{name}({pn}): default {got}, reference {default}")
            for pn, p in mine[len(params):]:
                if p.default is inspect.Parameter.empty:
                    problems.append(f"{qual}.{name}: extra required parameter {pn!r}")
    assert not problems, "\n".join(problems)


def test_no_pos_fails_like_the_reference():
    """encoder.py:165-166 selects NoPositionalEncoding, a name the reference never defines: NameError there and here."""
    from openeat_amd.modules.encoder import TransformerEncoder
    with pytest.raises(NameError):
        TransformerEncoder(80, pos_enc_layer_type="no_pos", d_model=16, attention_heads=4, linear_units=32, num_blocks=1)


def test_pad_targets_and_cut_are_inert_on_the_host():
    """engine.pad_targets pads label matrices with ignore_id to a multiple (fewer distinct shapes for step_cached);
    ops.cut is the identity unless a segmented capture is recording cut points."""
    import torch
    from openeat_amd import ops
    from openeat_amd.engine import pad_targets
    t = torch.tensor([[3, 4, 5], [6, -1, -1]], dtype=torch.int32)
    p = pad_targets(t, 4)
    assert p.shape == (2, 4) and p.dtype == t.dtype and p[:, :3].equal(t) and p[:, 3].tolist() == [-1, -1]
    assert pad_targets(p, 4) is p
    x = torch.ones(2, 3, requires_grad=True) * 2
    assert ops.CUTS is None and ops.cut(x, "heads") is x
    ops.CUTS = []
    try:
        y = ops.cut(x, "heads")
        assert y is not x and y.requires_grad and y.grad_fn is None and torch.equal(y, x) and ops.CUTS[0][0] == "heads"
        assert ops.cut(x.detach(), "enc3").requires_grad is False and len(ops.CUTS) == 1       # nothing to cut on a constant
    finally:
        ops.CUTS = None


def test_get_subsample_matches_reference_table():
    """utils/common.py:176-184."""
    from openeat_amd.utils.common import get_subsample
    for layer, want in (("conv2d", 4), ("conv2d6", 6), ("conv2d8", 8)):
        assert get_subsample({"encoder_conf": {"input_layer": layer}}) == want
    import pytest
    with pytest.raises(AssertionError):
        get_subsample({"encoder_conf": {"input_layer": "linear"}})


def test_mask_bytes_views_a_bool_mask_and_converts_the_rest():
    """ops.mask_bytes: the masks of encoder_layer.py:86-95 / decoder.py:167-194 as uint8 without a conversion launch."""
    from openeat_amd import ops
    m = torch.tensor([[[True, False, True, True]], [[False, False, True, True]]])
    b = ops.mask_bytes(m)
    assert b.dtype == torch.uint8 and b.data_ptr() == m.data_ptr() and b.tolist() == m.int().tolist()
    t = m.transpose(0, 2)                                   # not contiguous: copied, then viewed
    assert ops.mask_bytes(t).is_contiguous() and ops.mask_bytes(t).tolist() == t.int().tolist()
    i = m.to(torch.int64)
    assert ops.mask_bytes(i).dtype == torch.uint8 and ops.mask_bytes(i).tolist() == i.tolist()
    u = m.to(torch.uint8)
    assert ops.mask_bytes(u).data_ptr() == u.data_ptr()


def test_capture_scope_isolates_the_planes_registry_on_the_host():
    """planes.capture_scope (host logic only, no device): inside the scope the registry starts empty and cached weight splits
    are neither read nor written; on exit the capture's entries are gone and the outer registry object is back (round 3's red
    GPU test: a capture baked in planes that the eager FIFO later freed)."""
    from openeat_amd import planes
    planes.clear_all()
    src = torch.zeros(4, 8)
    pl = planes.Planes(torch.zeros(3, 4, 8, dtype=torch.bfloat16), 0, 32, 8, 4, 8)
    planes._REG[1234] = (pl, src, src._version)
    outer = planes._REG
    with planes.capture_scope():
        assert planes._REG is not outer and len(planes._REG) == 0 and planes._CAPTURE_DEPTH == 1
        planes._REG[99] = (pl, src, src._version)
        with planes.capture_scope():                          # nests (a segmented capture inside an engine capture)
            assert len(planes._REG) == 0 and planes._CAPTURE_DEPTH == 2
        assert 99 in planes._REG
    assert planes._REG is outer and list(outer) == [1234] and planes._CAPTURE_DEPTH == 0
    try:
        with planes.capture_scope():
            raise KeyError("boom")
    except KeyError:
        pass
    assert planes._REG is outer and planes._CAPTURE_DEPTH == 0
    planes.clear_all()
    assert len(planes._REG) == 0 and len(planes._WCACHE) == 0


def test_gpu_files_are_collected_kernel_proofs_first():
    """One failing integration test must not hide the kernel-level evidence under the driver's `pytest -x`."""
    import conftest
    order = conftest._GPU_FILE_ORDER
    for early in ("test_gpu_kernels.py", "test_gpu_planes.py", "test_gpu_width.py"):
        assert order.index(early) < order.index("test_gpu_model.py") < order.index("test_gpu_engine.py")
    here = os.path.dirname(os.path.abspath(__file__))
    present = sorted(f for f in os.listdir(here) if f.startswith("test_gpu_") and f.endswith(".py"))
    assert set(present) <= set(order), f"add {set(present) - set(order)} to conftest._GPU_FILE_ORDER"


def test_pack_table_dead_row_predicates():
    """ops._row_dead / ops._ffn_dead (host logic only): a packed-weight row is dead when its owner is gone OR when the owner lives
    on at another address (`p.data = ...`: ParamArena, load_state_dict-style re-pointing) - a sweep that looked at the owner's
    life alone kept refreshing from the freed old storage.  Only the untouched rows survive a sweep."""
    import gc
    import weakref
    from openeat_amd import ops

    def row_ent(p):
        return dict(owner=weakref.ref(p), off=0)

    ps = {name: torch.nn.Parameter(torch.randn(8, 8)) for name in ("deleted", "repointed", "untouched")}
    tab = ops._PackTable(6)
    keys = {}
    for name, p in ps.items():
        keys[name] = (p.data_ptr(), 8, 8, 8, 0)
        assert tab.add(keys[name], [p.data_ptr(), 0, 8, 8, 8, 0], row_ent(p), "cpu")
    # (a view's row: its source address sits `off` bytes into the owner)
    keys["view"] = (ps["untouched"].data_ptr() + 4 * 8, 7, 8, 8, 0)
    assert tab.add(keys["view"], [keys["view"][0], 0, 7, 8, 8, 0], dict(owner=weakref.ref(ps["untouched"]), off=4 * 8), "cpu")
    assert not any(ops._row_dead(k, tab.entries[k]) for k in keys.values())
    del ps["deleted"]
    gc.collect()
    moved = ps["repointed"]
    moved.data = torch.randn(8, 8)                         # a live Parameter whose storage moved
    assert moved.data_ptr() != keys["repointed"][0]
    assert ops._row_dead(keys["deleted"], tab.entries[keys["deleted"]])
    assert ops._row_dead(keys["repointed"], tab.entries[keys["repointed"]])
    assert not ops._row_dead(keys["untouched"], tab.entries[keys["untouched"]])
    assert not ops._row_dead(keys["view"], tab.entries[keys["view"]])
    tab.sweep(ops._row_dead)
    assert set(tab.entries) == {keys["untouched"], keys["view"]}
    live = {int(tab.host[i, 0]) for i in range(tab.n) if int(tab.host[i, 0])}
    assert live == {keys["untouched"][0], keys["view"][0]}     # the dead rows are neutralised (source pointer 0), not removed
    assert tab.n == 4

    w = {name: (torch.nn.Parameter(torch.randn(16, 8)), torch.nn.Parameter(torch.randn(8, 16))) for name in ("deleted", "repointed", "untouched")}
    ftab = ops._PackTable(9)
    fkeys = {}
    for name, (w1, w2) in w.items():
        fkeys[name] = (w1.data_ptr(), w2.data_ptr(), 6)
        assert ftab.add(fkeys[name], [w1.data_ptr(), w2.data_ptr(), 0, 0, 0, 0, 8, 16, 3], dict(w1=weakref.ref(w1), w2=weakref.ref(w2)), "cpu")
    del w["deleted"]
    gc.collect()
    w["repointed"][1].data = torch.randn(8, 16)            # W2 alone moves: the row is dead all the same
    for name, dead in (("deleted", True), ("repointed", True), ("untouched", False)):
        assert ops._ffn_dead(fkeys[name], ftab.entries[fkeys[name]]) == dead, name
    ftab.sweep(ops._ffn_dead)
    assert set(ftab.entries) == {fkeys["untouched"]}
    assert [int(ftab.host[i, 0]) for i in range(ftab.n)] == [0, 0, fkeys["untouched"][0]]


def test_parked_layernorm_entries_and_reduce_table(monkeypatch):
    """ops._LnFwdPark / _LnBwdPark / _ParkRegistry / _ln_param_reduce (host logic only, hip.call recorded): resolve() of a single
    and a pair entry, forward and backward, issues exactly the separate launches - names and argument order - and nothing the second
    time; a backward parked in table mode records its rows at once and reduces nothing when launched; sweep() launches what is not
    done and empties the registry; a parameter-gradient reduce is a table row in table mode (arena gradients only), else a launch."""
    from openeat_amd import hip, ops, planes
    calls = []
    monkeypatch.setattr(hip, "call", lambda name, *args: calls.append((name,) + args))
    monkeypatch.setattr(planes, "POLICY", "conv")                  # (no pre-split operands: the plain LayerNorm forward)
    monkeypatch.setattr(ops, "_seed_dev", torch.zeros(1, dtype=torch.int64))
    monkeypatch.setattr(ops, "LN_TABLE", None)
    sd = ops._seed_dev

    def expect(*want):
        got = calls[:]
        calls.clear()
        same = lambda a, b: a is b if any(v is None or isinstance(v, torch.Tensor) for v in (a, b)) else a == b
        assert len(got) == len(want), got
        for c, w in zip(got, want):
            assert c[0] == w[0] and len(c) == len(w) and all(same(a, b) for a, b in zip(c[1:], w[1:])), (c[0], w[0])

    rows, d = 6, 8
    x, dy, add, u, y, g, dx = (torch.zeros(rows, d) for _ in range(7))
    g1, b1, g2, b2, dg1, db1, dg2, db2 = (torch.zeros(d) for _ in range(8))
    st1, st2, mask, gmask, ws1, ws2 = torch.zeros(rows, 2), torch.zeros(rows, 2), torch.ones(rows), torch.ones(rows), torch.zeros(64), torch.zeros(64)
    spec = (0.5, 0.1, 1234, gmask)

    single = ops._LnFwdPark(x, g1, b1, 1e-5, rows, d, y, st1, rowmask=mask)
    pair = ops._LnFwdPark(x, g1, b1, 1e-5, rows, d, y, st1, gamma2=g2, beta2=b2, eps2=1e-6, u=u, stats2=st2)
    for e in (single, single, pair, pair):
        e.resolve()
    expect(("oe_layernorm_fwd", x, g1, b1, 1e-5, rows, d, mask, 0, y, st1),
           ("oe_layernorm_pair_fwd", x, g1, b1, 1e-5, g2, b2, 1e-6, rows, d, u, st1, y, st2))
    assert single.done and pair.done

    def bwd(g_=g, pair_=False):
        if pair_:
            return ops._LnBwdPark(dy, x, g1, b1, st1, add, dx, g_, ws1, spec, rows, d, dg1, db1, gamma2=g2, stats2=st2, ws2=ws2, dg2=dg2, db2=db2)
        return ops._LnBwdPark(dy, x, g1, b1, st1, add, dx, g_, ws1, spec, rows, d, dg1, db1, rowmask=mask)

    single, pair = bwd(), bwd(pair_=True)
    for e in (single, single, pair, pair):
        e.resolve()
    expect(("oe_layernorm_bwd_dx_drop", dy, x, g1, b1, 0, st1, rows, d, mask, add, dx, g, 0.5, 0.1, 1234, sd, gmask, ws1),
           ("oe_layernorm_param_reduce", ws1, rows, d, dg1, db1),
           ("oe_layernorm_pair_bwd_dx_drop", dy, x, g1, b1, st1, g2, st2, rows, d, add, dx, g, 0.5, 0.1, 1234, sd, gmask, ws1, ws2),
           ("oe_layernorm_param_reduce", ws1, rows, d, dg1, db1), ("oe_layernorm_param_reduce", ws2, rows, d, dg2, db2))
    n0 = ops.LN_BWD_FUSED_LAUNCHES
    bwd(pair_=True).fused()
    expect(("oe_layernorm_param_reduce", ws1, rows, d, dg1, db1), ("oe_layernorm_param_reduce", ws2, rows, d, dg2, db2))
    assert ops.LN_BWD_FUSED_LAUNCHES == n0 + 1

    # table mode: the rows go in when the entry is parked, whatever happens later
    table = ops._LnTable(torch.zeros(8, 5, dtype=torch.int64), eager=False)
    monkeypatch.setattr(ops, "LN_TABLE", table)
    parked = bwd(pair_=True)
    assert table.entries == [(ws1.data_ptr(), rows, d, dg1.data_ptr(), db1.data_ptr()), (ws2.data_ptr(), rows, d, dg2.data_ptr(), db2.data_ptr())]
    assert table.keep == [ws1, ws2] and (table.max_rows, table.max_d) == (rows, d)
    parked.resolve()
    parked.fused()
    expect(("oe_layernorm_pair_bwd_dx_drop", dy, x, g1, b1, st1, g2, st2, rows, d, add, dx, g, 0.5, 0.1, 1234, sd, gmask, ws1, ws2))
    ops._ln_param_reduce(ws1, 2 * rows, 2 * d, dg1, db1, True)
    assert len(table.entries) == 3 and table.keep[-1] is ws1 and (table.max_rows, table.max_d) == (2 * rows, 2 * d)
    expect()
    ops._ln_param_reduce(ws1, rows, d, dg1, db1, False)
    monkeypatch.setattr(ops, "LN_TABLE", None)
    ops._ln_param_reduce(ws2, rows, d, dg2, db2, True)
    expect(("oe_layernorm_param_reduce", ws1, rows, d, dg1, db1), ("oe_layernorm_param_reduce", ws2, rows, d, dg2, db2))
    assert len(table.entries) == 3

    # the registry: keyed by the parked output, take() removes, sweep() launches what nobody launched
    reg = ops._ParkRegistry("g")
    monkeypatch.setattr(ops, "_PENDING_LN", reg)
    gs = [torch.zeros(rows, d) for _ in range(4)]
    entries = [bwd(g_) for g_ in gs]
    for e in entries:
        reg.park(e)
    assert len(reg) == 4 and reg.take(torch.zeros(rows, d)) is None and reg.take(gs[0]) is entries[0] and reg.take(gs[0]) is None
    entries[1].resolve()
    calls.clear()
    assert ops.resolve_pending_ln() == 2 and not reg and reg.take(gs[2]) is None
    assert [c[0] for c in calls] == ["oe_layernorm_bwd_dx_drop", "oe_layernorm_param_reduce"] * 2
    assert calls[0][12] is gs[2] and calls[2][12] is gs[3]
    calls.clear()
    assert reg.sweep() == 0 and not calls and not entries[0].done
