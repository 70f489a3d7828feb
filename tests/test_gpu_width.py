"""GPU: the WHOLE model at the benchmarked width against the CPU oracle - BASELINE.json configs[1]'s 12-layer Conformer
(d=256, h=4, ff=1024, K=15, 12+3+3, V=3246), dropout 0, on bench.py's synthetic batch (uniform-noise wav through the
device fbank) with ragged utterance lengths, ragged target lengths and one short utterance.  At this width the GEMMs run
the interior 128x128 / 64x64 straight-line tiles, the LDS-DMA ring and the split-K paths that bench.py times - the d=32
goldens only reach the bounds-checked edge tiles.

Run in both arithmetic modes: precision 0 (exact-fp32 matrix products) and precision 3 (bf16x3 on the matrix cores, the
mode bench.py reports).  Tolerances: loss rtol 2e-4; every parameter-gradient norm within 3e-3
relative (floor 1e-6 absolute: Adam-irrelevant parameters such as the key bias have true gradient ~0); CTC-greedy token
ids identical to the oracle's on every utterance.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from openeat_amd.frontend import Fbank, utt_normalize_  # noqa: E402
from openeat_amd.models.asr_model import ASRModel  # noqa: E402
from oracle import asr as O  # noqa: E402

DEV = "cuda"
V = 3246
CONF = dict(encoder_num_blocks=12, decoder_num_blocks=3, r_decoder_num_blocks=3, d_model=256, attention_heads=4,
            linear_units=1024, dropout_rate=0.0, input_layer="conv2d", pos_enc_layer_type="rel_pos", activation_type="swish",
            macaron_style=True, use_cnn_module=True, cnn_module_kernel=15, causal=False, ctc_weight=0.3, lsm_weight=0.1,
            reverse_weight=0.3, length_normalized_loss=False)
SECONDS = [10.0, 9.4, 8.7, 7.5, 6.2, 5.6, 10.0, 1.5]            # ragged; the last one is the short utterance
TLENS = [30, 27, 25, 22, 18, 16, 30, 4]

# bench.py's own batch size: 32 utterances, 7936 encoder rows once the eight 10 s ones pad the rest - the row count at which the
# dispatch picks the tiles / kernels the benchmark times (128 x 128 ring tiles for the wide outputs, 128 x 64 for the long narrow
# reductions, the grouped weight gradients, the conv front end's pre-split GEMMs with their full-size grids)
SECONDS32 = [10.0] * 8 + [9.9 - 0.23 * i for i in range(23)] + [1.5]
TLENS32 = [30] * 8 + [29 - i for i in range(23)] + [4]

_CACHES = {}


def _synth_batch(seconds, tlens):
    """bench.py::synth_batch's uniform-noise wav through the device fbank, and random targets: (feats, nfr, tgt, tlen)."""
    g = torch.Generator().manual_seed(0)
    B = len(seconds)
    ns = torch.tensor([int(16000 * s) for s in seconds])
    wav = torch.rand(B, int(ns.max()), generator=g) - 0.5
    tgt = torch.full((B, max(tlens)), -1, dtype=torch.int32)
    for b in range(B):
        wav[b, int(ns[b]):] = 0.0
        tgt[b, : tlens[b]] = torch.randint(2, V - 1, (tlens[b],), generator=g, dtype=torch.int32)
    tlen = torch.tensor(tlens, dtype=torch.int32)
    feats, nfr = Fbank(80, device=DEV)(wav.to(DEV), ns.to(DEV))
    utt_normalize_(feats, nfr)
    torch.cuda.synchronize()
    assert nfr.tolist()[0] == 998 and nfr.tolist()[-1] == 148
    return feats, nfr, tgt, tlen


def _setup(seconds=None, tlens=None):
    seconds, tlens = seconds or SECONDS, tlens or TLENS
    _CACHE = _CACHES.setdefault(len(seconds), {})
    if _CACHE:
        return _CACHE
    torch.manual_seed(777)
    model = ASRModel(80, V, **CONF)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    feats, nfr, tgt, tlen = _synth_batch(seconds, tlens)
    # the oracle on the same features (CPU, a few seconds)
    cfg = O.Config(input_size=80, vocab_size=V, **CONF)
    osd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    loss, acc = O.forward(osd, cfg, feats.cpu(), nfr.cpu(), tgt, tlen)
    loss.backward()
    greedy = O.ctc_greedy_search({k: v.detach() for k, v in osd.items()}, cfg, feats.cpu(), nfr.cpu())
    _CACHE.update(sd=sd, feats=feats, nfr=nfr, tgt=tgt, tlen=tlen, loss=float(loss), acc=float(acc), greedy=greedy,
                  gnorm={k: float(v.grad.norm()) for k, v in osd.items() if v.grad is not None},
                  gctc=osd["ctc.ctc_lo.weight"].grad.clone(), gemb=osd["encoder.embed.conv.0.weight"].grad.clone())
    return _CACHE


@pytest.mark.parametrize("prec,fused_ffn,full", [(0, False, False), (6, False, False), (60, False, False), (3, False, False), (3, True, False),
                                                  (6, False, True), (61, False, True), (6, True, False), (6, True, True)],
                         ids=["fp32-mfma", "bf16x6-mfma", "bf16x6-planes-forced", "bf16x3-mfma", "bf16x3-mfma-fused-ffn",
                              "bf16x6-mfma-B32", "bf16x6-planes-ln-B32", "bf16x6-mfma-fused-ffn", "bf16x6-mfma-fused-ffn-B32"])
def test_config2_width_model_matches_oracle(prec, fused_ffn, full):
    """fused_ffn: the one-kernel feed forward (csrc/ffn.hip) forced on at this batch's 1984 rows (by default it takes over from
    4096 rows on, i.e. at bench.py's batch) - the same tolerances end to end.  full: bench.py's batch size (32 utterances, 7936
    encoder rows) in the headline arithmetic, so that exactly the kernels / tiles the benchmark times are the ones checked;
    61 = precision 6 with the "ln" pre-split policy (LayerNorm outputs + arena-free weight planes)."""
    from openeat_amd import hip, ops
    c = _setup(SECONDS32, TLENS32) if full else _setup()
    old_min, ops.FUSED_FFN_MIN_ROWS = ops.FUSED_FFN_MIN_ROWS, (0 if fused_ffn else 1 << 30)
    old_bwd, ops.FUSED_FFN_BWD = ops.FUSED_FFN_BWD, bool(fused_ffn)          # the one-launch input gradient rides along when forced
    model = ASRModel(80, V, **CONF)
    model.load_state_dict(c["sd"])
    model = model.to(DEV).eval()
    from openeat_amd import planes
    old, old_pmin, old_pol = hip.GEMM_PRECISION, planes.MIN_SPLIT_ELEMS, planes.POLICY
    hip.GEMM_PRECISION = 6 if prec in (60, 61) else prec
    if prec == 60:
        planes.MIN_SPLIT_ELEMS, planes.POLICY = 0, "all"   # every operand pre-split: gemm_pl.hip wherever the shapes qualify
        hip.lib().oe_gemm_pl_config(0, -1, -1, -1)
    if prec == 61:
        planes.POLICY = "ln"
    try:
        loss, acc = model(c["feats"], c["nfr"], c["tgt"].to(DEV), c["tlen"].to(DEV))
        loss.backward()
        with torch.no_grad():
            greedy = model.ctc_greedy_search(c["feats"], c["nfr"])
        torch.cuda.synchronize()
    finally:
        hip.GEMM_PRECISION, planes.MIN_SPLIT_ELEMS, planes.POLICY = old, old_pmin, old_pol
        hip.lib().oe_gemm_pl_config(96, 0, 0, 8)
        planes.clear()
        ops.FUSED_FFN_MIN_ROWS = old_min
        ops.FUSED_FFN_BWD = old_bwd
    assert abs(float(loss) - c["loss"]) <= 2e-4 * abs(c["loss"]), (float(loss), c["loss"])
    assert abs(float(acc) - c["acc"]) <= 1e-6
    bad = []
    for k, p in model.named_parameters():
        want = c["gnorm"][k]
        got = float(p.grad.norm())
        if abs(got - want) > 3e-3 * abs(want) + 1e-6:
            bad.append((k, got, want))
    assert not bad, bad[:10]
    # element-wise on the two ends of the network: the last layer's weight gradient and the first conv's
    for key, ref in (("ctc.ctc_lo.weight", c["gctc"]), ("encoder.embed.conv.0.weight", c["gemb"])):
        got = dict(model.named_parameters())[key].grad.cpu()
        assert float((got - ref).abs().max()) <= 3e-3 * float(ref.abs().max()), key
    assert greedy == c["greedy"]                                   # bit-exact CTC-greedy ids on every utterance
    assert sum(len(h) for h in greedy) > 0


def test_config2_width_training_trajectory_matches_oracle():
    """Eight optimizer steps of the bench's step machinery - captured HIP graph (grouped weight gradients,
    clip + fused Adam inside), precision 6 - against the oracle's forward / backward / clip_grad_norm_ / torch.optim.Adam on the
    CPU from the same initial weights on the same batch (dropout 0): the LOSS TRAJECTORY, not one step.  Adam's first steps
    move every weight by ~lr whatever the gradient's size, so arithmetic differences do compound; measured agreement is ~1e-5
    relative at every step (617.34 -> 143.53 over eight steps), the test holds it to the single-step tolerance 2e-4."""
    from openeat_amd import hip, ops
    from openeat_amd.engine import TrainEngine
    c = _setup()
    n_steps, lr, B = 8, 1e-3, 4                                   # the first four utterances: ~1000 encoder rows, seconds per CPU step
    feats, nfr = c["feats"][:B].contiguous(), c["nfr"][:B].contiguous()
    tgt, tlen = c["tgt"][:B].contiguous(), c["tlen"][:B].contiguous()
    cfg = O.Config(input_size=80, vocab_size=V, **CONF)
    osd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in c["sd"].items()}
    params = [v for v in osd.values() if v.requires_grad]
    opt = torch.optim.Adam(params, lr=lr)
    want = []
    for _ in range(n_steps):
        loss, _ = O.forward(osd, cfg, feats.cpu(), nfr.cpu(), tgt, tlen)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        want.append(float(loss))
    model = ASRModel(80, V, **CONF)
    model.load_state_dict(c["sd"])
    model = model.to(DEV).train()
    old = hip.GEMM_PRECISION
    hip.GEMM_PRECISION = 6                                        # bench.py's arithmetic
    eng = TrainEngine(model, lr=lr, grad_clip=5.0, static_shapes=True, parallel_decoders=True)
    batch = dict(features=feats, features_length=nfr, targets=tgt.to(DEV), targets_length=tlen.to(DEV))
    got = []
    try:
        got.append(float(eng.step(batch)[0]))                       # step 1 eager
        eng.capture(batch, warmup=1)                                # step 2 = the capture's warm-up step (a real step)
        got.append(None)
        for _ in range(n_steps - 2):
            got.append(float(eng.replay()[0]))                      # steps 3.. from the graph
        torch.cuda.synchronize()
    finally:
        hip.GEMM_PRECISION = old
        eng.arena.deactivate()
        ops.set_seed_device_counter(None)
        ops.PARALLEL_DECODERS = False
        ops.POS_PROJ_AHEAD = False
    print("trajectory oracle:", [round(w, 4) for w in want], "hip:", [None if g is None else round(g, 4) for g in got])
    assert want[-1] < 0.8 * want[0], want                           # the model is really learning this batch
    for i, (g, w) in enumerate(zip(got, want)):
        if g is not None:
            assert abs(g - w) <= 2e-4 * abs(w), (i, got, want)


# ---- the training trajectory at the rows where the row-block GEMMs, the fused feed-forward, the LayerNorm prologues / epilogue and
# the packed-weight tables engage (d = 256, precision 6, >= 4096 encoder rows: ops.ROWGEMM_MIN_ROWS, ops.FUSED_FFN_MIN_ROWS) ----------
# CONF's widths on a shallower model (which kernels engage depends on d and rows, not depth): the CPU oracle stays cheap
CONF_SHALLOW = dict(CONF, encoder_num_blocks=4, decoder_num_blocks=1, r_decoder_num_blocks=1)
SECONDS18 = [10.0] * 2 + [9.8 - 0.5 * i for i in range(15)] + [1.5]     # 18 x 248 = 4464 encoder rows; the last one is short
TLENS18 = [30] * 2 + [29 - i for i in range(15)] + [4]
TRAJ_STEPS, TRAJ_LR = 6, 1e-3
_TRAJ = {}


def _setup_trajectory():
    """Initial weights, the batch and the oracle's loss trajectory (forward / backward / clip_grad_norm_ / torch.optim.Adam on the
    CPU, dropout 0): TRAJ_STEPS steps."""
    import time
    if _TRAJ:
        return _TRAJ
    torch.manual_seed(779)
    model = ASRModel(80, V, **CONF_SHALLOW)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    feats, nfr, tgt, tlen = _synth_batch(SECONDS18, TLENS18)
    cfg = O.Config(input_size=80, vocab_size=V, **CONF_SHALLOW)
    osd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    params = [v for v in osd.values() if v.requires_grad]
    opt = torch.optim.Adam(params, lr=TRAJ_LR)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    t0 = time.perf_counter()
    want = []
    for _ in range(TRAJ_STEPS):
        loss, _ = O.forward(osd, cfg, feats.cpu(), nfr.cpu(), tgt, tlen)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        want.append(float(loss))
    cpu_s = time.perf_counter() - t0
    print(f"trajectory oracle: {TRAJ_STEPS} steps in {cpu_s:.1f} s on {torch.get_num_threads()} threads")
    _TRAJ.update(sd=sd, feats=feats, nfr=nfr, tgt=tgt, tlen=tlen, want=want, cpu_s=cpu_s)
    return _TRAJ


_PACK_COUNTERS = ("LN_FWD_FUSED_LAUNCHES", "LN_BWD_FUSED_LAUNCHES", "LN_EPI_FUSED_LAUNCHES", "ROWGEMM_LAUNCHES", "FFN_FWD_FUSED_LAUNCHES",
                  "FFN_BWD_FUSED_LAUNCHES")


def _trajectory_model(c):
    """The model in precision 6 after ONE no-grad pass at the batch's rows (a CTC-greedy decode): the packed-weight tables hold rows
    at the Parameters' own addresses before anything re-points them - the real-world order (a decode before training)."""
    from openeat_amd import ops
    model = ASRModel(80, V, **CONF_SHALLOW)
    model.load_state_dict(c["sd"])
    model = model.to(DEV).eval()
    with torch.no_grad():
        model.ctc_greedy_search(c["feats"], c["nfr"])
    torch.cuda.synchronize()
    assert ops._ROW.entries and ops._FFN.entries, "the decode registered no packed weights: the rows are below the kernels' threshold"
    return model.train()


def _count_parked_layernorms(monkeypatch):
    """Wrap ops.resolve_pending_ln / resolve_pending_lnf: the list receives every count of parked LayerNorms they had to launch
    late (a non-zero count after a step means some consumer read the LayerNorm's output before it was written)."""
    from openeat_amd import ops
    late = []
    for name in ("resolve_pending_ln", "resolve_pending_lnf"):
        def wrapped(orig=getattr(ops, name), name=name):
            n = orig()
            late.append((name, n))
            return n
        monkeypatch.setattr(ops, name, wrapped)
    return late


def _flush_parked(late):
    from openeat_amd import ops
    ops.resolve_pending_ln()
    ops.resolve_pending_lnf()
    late.clear()


def _assert_nothing_parked(late, what):
    from openeat_amd import ops
    ops.resolve_pending_ln()                                       # the sweep, now: what did the step leave?
    ops.resolve_pending_lnf()
    assert all(n == 0 for _, n in late), (what, late)
    late.clear()


def _restore(old_prec):
    from openeat_amd import hip, ops
    hip.GEMM_PRECISION = old_prec
    ops.set_seed_device_counter(None)
    ops.PARALLEL_DECODERS = False
    ops.POS_PROJ_AHEAD = False


def test_config2_width_training_trajectory_at_bench_rows_matches_oracle(monkeypatch):
    """TrainEngine (static shapes, parallel decoders, precision 6) at 4464 encoder rows after a decode registered the packs: one
    eager step, capture (its warm-up step is real), three replays, drop the graph (empty_cache), one more eager step - every
    observable loss within 2e-4 relative of the oracle's trajectory.  The packed-weight tables hold no row of freed storage after
    the engine re-points the weights nor after the graph's memory went back (tests/packcheck.py, checked before any launch)."""
    from openeat_amd import hip, ops, planes
    from openeat_amd.engine import TrainEngine
    from packcheck import assert_pack_rows_live
    c = _setup_trajectory()
    late = _count_parked_layernorms(monkeypatch)
    old = hip.GEMM_PRECISION
    hip.GEMM_PRECISION = 6
    batch = dict(features=c["feats"], features_length=c["nfr"], targets=c["tgt"].to(DEV), targets_length=c["tlen"].to(DEV))
    got, moved = [], None
    eng = None
    try:
        model = _trajectory_model(c)
        eng = TrainEngine(model, lr=TRAJ_LR, grad_clip=5.0, static_shapes=True, parallel_decoders=True)
        planes.new_pass()
        assert_pack_rows_live()
        _flush_parked(late)                                        # (what the decode left: not a training step)
        c0 = {k: getattr(ops, k) for k in _PACK_COUNTERS}
        got.append(float(eng.step(batch)[0]))                      # step 1: eager
        moved = {k: getattr(ops, k) - c0[k] for k in _PACK_COUNTERS}
        _assert_nothing_parked(late, "eager step 1")
        eng.capture(batch, warmup=1)                               # step 2: the capture's warm-up step (a real step)
        got.append(None)
        for _ in range(3):
            got.append(float(eng.replay()[0]))                     # steps 3-5 from the graph
        torch.cuda.synchronize()
        eng.drop_graph()                                           # (torch.cuda.empty_cache: freed storage may be unmapped now)
        planes.new_pass()
        assert_pack_rows_live()
        got.append(float(eng.step(batch)[0]))                      # step 6: eager again
        torch.cuda.synchronize()
        _assert_nothing_parked(late, "eager step 6")
    finally:
        _restore(old)
        if eng is not None:
            eng.arena.deactivate()
    want = c["want"]
    rel = [None if g is None else abs(g - w) / abs(w) for g, w in zip(got, want)]
    print("trajectory at 4464 rows: oracle", [round(w, 4) for w in want], "hip", [None if g is None else round(g, 4) for g in got],
          "rel", [None if r is None else f"{r:.2e}" for r in rel], f"oracle CPU {c['cpu_s']:.1f} s")
    assert all(v > 0 for v in moved.values()), moved               # the kernels under test really ran in the eager step
    assert want[-1] < 0.8 * want[0], want                          # the model is really learning this batch
    for i, r in enumerate(rel):
        assert r is None or r <= 2e-4, (i, got, want)


def test_config2_width_reference_loop_at_bench_rows_matches_oracle(monkeypatch):
    """The reference-shaped loop outside the engine (ParamArena + FusedAdam + model(**batch) + backward()) at the same rows, after
    the same decode: the packs follow the arena's re-pointing and the optimizer's raw writes - losses on the oracle's trajectory."""
    from openeat_amd import hip, ops, planes
    from openeat_amd.arena import ParamArena
    from openeat_amd.optim import FusedAdam
    from packcheck import assert_pack_rows_live
    c = _setup_trajectory()
    late = _count_parked_layernorms(monkeypatch)
    old = hip.GEMM_PRECISION
    hip.GEMM_PRECISION = 6
    batch = dict(features=c["feats"], features_length=c["nfr"], targets=c["tgt"].to(DEV), targets_length=c["tlen"].to(DEV))
    got, ar = [], None
    try:
        model = _trajectory_model(c)
        ar = ParamArena(model).activate()
        opt = FusedAdam(ar, lr=TRAJ_LR, max_grad_norm=5.0)
        planes.new_pass()
        assert_pack_rows_live()
        _flush_parked(late)                                        # (what the decode left: not a training step)
        for step in range(4):
            opt.zero_grad()
            loss, _ = model(**batch)
            loss.backward()
            ops.join_side_stream()
            opt.step()
            got.append(float(loss))
            _assert_nothing_parked(late, f"step {step + 1}")
        torch.cuda.synchronize()
    finally:
        _restore(old)
        if ar is not None:
            ar.deactivate()
    want = c["want"][:len(got)]
    print("reference loop at 4464 rows: oracle", [round(w, 4) for w in want], "hip", [round(g, 4) for g in got])
    for i, (g, w) in enumerate(zip(got, want)):
        assert abs(g - w) <= 2e-4 * abs(w), (i, got, want)


# ---- BASELINE.json configs[4]'s model: 24-layer Conformer d = 512 (h = 8, ff = 2048, K = 15; SURVEY 8d's assumed widths) ----------
CONF5 = dict(CONF, encoder_num_blocks=24, d_model=512, attention_heads=8, linear_units=2048)
SECONDS5 = [4.0, 3.1, 2.3, 1.5]
TLENS5 = [14, 11, 8, 4]
_C5 = {}


def _setup5():
    if _C5:
        return _C5
    torch.manual_seed(778)
    model = ASRModel(80, V, **CONF5)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    B = len(SECONDS5)
    ns = torch.tensor([int(16000 * s) for s in SECONDS5])
    wav = torch.rand(B, int(ns.max()), generator=g) - 0.5
    tgt = torch.full((B, max(TLENS5)), -1, dtype=torch.int32)
    for b in range(B):
        wav[b, int(ns[b]):] = 0.0
        tgt[b, : TLENS5[b]] = torch.randint(2, V - 1, (TLENS5[b],), generator=g, dtype=torch.int32)
    tlen = torch.tensor(TLENS5, dtype=torch.int32)
    feats, nfr = Fbank(80, device=DEV)(wav.to(DEV), ns.to(DEV))
    utt_normalize_(feats, nfr)
    torch.cuda.synchronize()
    cfg = O.Config(input_size=80, vocab_size=V, **CONF5)
    osd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    loss, acc = O.forward(osd, cfg, feats.cpu(), nfr.cpu(), tgt, tlen)
    loss.backward()
    greedy = O.ctc_greedy_search({k: v.detach() for k, v in osd.items()}, cfg, feats.cpu(), nfr.cpu())
    _C5.update(sd=sd, feats=feats, nfr=nfr, tgt=tgt, tlen=tlen, loss=float(loss), acc=float(acc), greedy=greedy,
               gnorm={k: float(v.grad.norm()) for k, v in osd.items() if v.grad is not None})
    return _C5


@pytest.mark.parametrize("prec,fused_ffn", [(6, False), (0, False), (6, True)], ids=["bf16x6-mfma", "fp32-mfma", "bf16x6-mfma-fused-ffn"])
def test_config5_width_model_matches_oracle(prec, fused_ffn):
    """The d = 512 dispatch (other tiles, K = 512 / 2048 reductions, eight heads of 64, 192.5 M parameters in one arena-less model)
    against oracle/asr.py on four ragged utterances: loss rtol 2e-4, every parameter-gradient norm 3e-3, CTC-greedy ids identical
    (asr_model.py:37-70 kwargs)."""
    from openeat_amd import hip, ops, planes
    c = _setup5()
    model = ASRModel(80, V, **CONF5)
    model.load_state_dict(c["sd"])
    model = model.to(DEV).eval()
    old = hip.GEMM_PRECISION
    hip.GEMM_PRECISION = prec
    old_ffn = (ops.FUSED_FFN_MIN_ROWS, ops.FUSED_FFN_BWD)
    if fused_ffn:                                    # csrc/ffn6.hip at d = 512, ff = 2048 (32-row blocks, two wave groups), forward and input gradient
        ops.FUSED_FFN_MIN_ROWS, ops.FUSED_FFN_BWD = 0, True
    try:
        loss, acc = model(c["feats"], c["nfr"], c["tgt"].to(DEV), c["tlen"].to(DEV))
        loss.backward()
        with torch.no_grad():
            greedy = model.ctc_greedy_search(c["feats"], c["nfr"])
        torch.cuda.synchronize()
    finally:
        hip.GEMM_PRECISION = old
        ops.FUSED_FFN_MIN_ROWS, ops.FUSED_FFN_BWD = old_ffn
        planes.clear()
    assert abs(float(loss) - c["loss"]) <= 2e-4 * abs(c["loss"]), (float(loss), c["loss"])
    assert abs(float(acc) - c["acc"]) <= 1e-6
    bad = []
    for k, p in model.named_parameters():
        want = c["gnorm"][k]
        got = float(p.grad.norm())
        if abs(got - want) > 3e-3 * abs(want) + 1e-6:
            bad.append((k, got, want))
    assert not bad, bad[:10]
    assert greedy == c["greedy"] and sum(len(h) for h in greedy) > 0
