"""Autograd-level composition of the HIP kernels.

Each ``torch.autograd.Function`` below is one block of the reference's hot path
(feed-forward, attention, conv module, subsampling, CTC head, label-smoothing
head ...) whose forward AND backward are sequences of C-ABI calls
(``openeat_amd.hip``).  PyTorch only owns the buffers and the tape.  No op
here has a CPU path: tensors must be float32 CUDA tensors.
"""
from __future__ import annotations

import itertools
import os
import math
import weakref
from typing import Optional

import torch

from . import hip
from . import arena as _arena
from . import planes as _planes

ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, ACT_HARDTANH, ACT_SELU, ACT_GELU = 0, 1, 2, 3, 4, 5, 6      # oe_common.h
ACT_IDS = {"relu": ACT_RELU, "swish": ACT_SWISH, "tanh": ACT_TANH, "hardtanh": ACT_HARDTANH, "selu": ACT_SELU, "gelu": ACT_GELU,
           "none": ACT_NONE}
# fused into GEMM epilogues; the others (never used by a shipped config) run as separate elementwise kernels so that
# their erf / tanh / exp code does not cost every GEMM kernel registers
GEMM_FUSED_ACTS = (ACT_NONE, ACT_RELU, ACT_SWISH)


# --------------------------------------------------------------------------- #
# dropout seeds: a host counter gives every dropout site a distinct stream; an
# optional device step counter (set by the training engine) is mixed in inside
# the kernels so that a captured HIP graph still draws fresh masks per replay.
# --------------------------------------------------------------------------- #
_seed_counter = itertools.count(0x5EED0001)
_seed_dev: Optional[torch.Tensor] = None


def next_seed() -> int:
    return next(_seed_counter) * 0x9E3779B1 & 0xFFFFFFFFFFFF


def set_seed_device_counter(t: Optional[torch.Tensor]):
    global _seed_dev
    _seed_dev = t


def manual_seed(seed: int):
    global _seed_counter
    _seed_counter = itertools.count(0x5EED0001 + (seed & 0xFFFFFFF) * 7919)


def _chk(t: torch.Tensor, name: str, keep_pending: bool = False) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{name}: openeat_amd ops need float32 CUDA tensors (got {t.dtype} on {t.device}); "
                        "there is no CPU fallback")
    if not keep_pending:
        # the output of a parked LayerNorm forward (PreNormFn) reaching an op that does not make it itself: launch it now
        pend = _PENDING_LNF.take(t)
        if pend is not None:
            pend.resolve()
    return t.contiguous()


class _ParkRegistry:
    """Parked LayerNorm launches (_LnFwdPark / _LnBwdPark) keyed by the address of their entry's output `attr` (forward y, backward g)."""

    def __init__(self, attr):
        self.attr, self._by_addr = attr, {}

    def __len__(self):
        return len(self._by_addr)

    def park(self, entry):
        self._by_addr[getattr(entry, self.attr).data_ptr()] = entry

    def take(self, t):
        """The entry parked on t's address (removed), or None."""
        return self._by_addr.pop(t.data_ptr(), None) if self._by_addr else None

    def sweep(self):
        """Launch every entry that nobody launched, forget them all; returns how many were launched."""
        late = [e for e in self._by_addr.values() if not e.done]
        for e in late:
            e.resolve()
        self._by_addr.clear()
        return len(late)


# The LayerNorm FORWARD of a pre-norm fork as the prologue of the GEMM that consumes it (oe_rowgemm6 / oe_ffn_fwd's lnf arguments):
# EncoderLayer promises (fuse_fwd) that the normed branch goes straight into an op of this module; PreNormFn.forward then parks the
# launch here, keyed by the address of its (still unwritten) output; the consumer's first kernel - the feed-forward, the fused
# q / k / v projection, the conv module's pointwise_conv1 - makes the rows on its way to LDS and writes y and the statistics for the
# backward.  Any other op of this module that receives a parked tensor launches the LayerNorm on its own first (_chk); leftovers are
# launched where the step's bookkeeping is reset (predrop_clear).  36 launches per step at config 2.
LN_FWD_FUSE = os.environ.get("OE_LN_FWD_FUSE", "1") == "1"
LN_FWD_FUSED_LAUNCHES = 0       # (tests)
_PENDING_LNF = _ParkRegistry("y")


def resolve_pending_lnf():
    return _PENDING_LNF.sweep()


class _LnFwdPark:
    """A parked LayerNorm forward: y = LN(x) (PreNormFn), or the pair form u = LN1(x), y = LN2(u) (NormPairFn)."""
    __slots__ = ("x", "gamma", "beta", "eps", "rows", "d", "y", "stats", "rowmask", "gamma2", "beta2", "eps2", "u", "stats2", "done")

    def __init__(self, x, gamma, beta, eps, rows, d, y, stats, rowmask=None, gamma2=None, beta2=None, eps2=None, u=None, stats2=None):
        self.x, self.gamma, self.beta, self.eps, self.rows, self.d, self.y, self.stats = x, gamma, beta, eps, rows, d, y, stats
        self.rowmask, self.gamma2, self.beta2, self.eps2, self.u, self.stats2 = rowmask, gamma2, beta2, eps2, u, stats2
        self.done = False

    def resolve(self):
        """The LayerNorm as a launch of its own (exactly what PreNormFn / NormPairFn.forward would have launched)."""
        if self.done:
            return
        self.done = True
        if self.gamma2 is not None:
            hip.call("oe_layernorm_pair_fwd", self.x, self.gamma, self.beta, self.eps, self.gamma2, self.beta2, self.eps2, self.rows, self.d,
                     self.u, self.stats, self.y, self.stats2)
        else:
            _ln_fwd(self.x, self.gamma, self.beta, self.eps, self.rows, self.d, self.rowmask, ACT_NONE, self.y, self.stats)

    def prologue(self):
        """The `lnf` argument of hip.rowgemm6 / hip.ffn_fwd (LnfPrologue.fill)."""
        return dict(x=self.x, gamma=self.gamma, beta=self.beta, eps=self.eps, y=self.y, stats=self.stats, rowmask=self.rowmask,
                    gamma2=self.gamma2, beta2=self.beta2, eps2=self.eps2, u=self.u, stats2=self.stats2)

    def fused(self):
        global LN_FWD_FUSED_LAUNCHES
        self.done = True
        LN_FWD_FUSED_LAUNCHES += 1


def _new(*shape, like: torch.Tensor, zero=False):
    return (torch.zeros if zero else torch.empty)(shape, device=like.device, dtype=torch.float32)


# --------------------------------------------------------------------------- #
# GEMM helpers
# --------------------------------------------------------------------------- #
def _split_k(out_rows: int, out_cols: int, k: int) -> int:
    """Split of the reduction dimension of a weight-gradient GEMM.  Large outputs use 128x128 tiles
    (fewer operand re-reads) with just enough splits to cover the 256 CUs; small ones 64x64 tiles with
    ~3 blocks per CU.  K-chunks stay >= 256 and the atomic traffic (splits x output bytes) bounded."""
    if hip.GEMM_PRECISION != 0 and out_rows >= 128 and out_cols >= 128:
        t128 = -(-out_rows // 128) * -(-out_cols // 128)
        sk = max(1, 256 // t128)          # at most one 128x128 block per CU (the ring kernel holds one per CU)
        if t128 * sk >= 200 and sk <= 24:
            return int(max(1, min(sk, k // 256 if k >= 512 else 1)))
    tiles = -(-out_rows // 64) * -(-out_cols // 64)
    want = max(1, 768 // max(tiles, 1))
    return int(max(1, min(want, 24, k // 256 if k >= 512 else 1)))


def _operand_planes(act2d, w2d):
    """Pre-split copies (planes.py) of an activation operand and a weight operand of one GEMM - both or neither."""
    if not _planes.active():
        # the weight alone, from the arena's planes (gemm_hyb.hip splits the activation on the fragment)
        return None, (_planes.arena_weight(w2d) if (_planes.weights_presplit() and act2d.shape[0] >= _planes.HYB_MIN_ROWS) else None)
    ap = _planes.of(act2d, make=_planes.split_activations())
    if ap is None:
        return None, None
    bp = _planes.weight(w2d)
    return (ap, bp) if bp is not None else (None, None)


# ---- the short-reduction Linears as row-block GEMMs (csrc/ffn6.hip::rowgemm6_kernel) ---------------------------------------
# x W^T and dy W with k in {256, 512} and an output width that is a multiple of 128, from ROWGEMM_MIN_ROWS rows on, in precision 6:
# the weight is consumed as packed fragments, refreshed for EVERY registered matrix by one table-driven launch per weights
# generation (as the feed-forwards' packs).  Anything the kernel's epilogue does not do stays on oe_gemm_f32.
ROWGEMM = os.environ.get("OE_ROWGEMM", "1") == "1"
ROWGEMM_MIN_ROWS = int(os.environ.get("OE_ROWGEMM_MIN_ROWS", "4096"))
ROWGEMM_LAUNCHES = 0       # (tests: which path a call took)
_ROW_EPI_OK = {"drop_p", "seed", "seed_dev", "rowmask", "residual", "ldr", "beta"}
# the tile form (few rows: oe_rowgemm6_form = 2, any k in {256, 512, 768, 1024}) also has oe_gemm_f32's activation epilogue
_ROWTILE_EPI_OK = _ROW_EPI_OK | {"act", "preact_out", "actgrad_in", "ld_aux"}
ROWTILE = os.environ.get("OE_ROWTILE", "1") == "1"


class _PackTable:
    """Device table of a table-driven pack launch (oe_rowgemm6_pack_table / oe_ffn_pack_weights_table) with the lifetime rules a
    CAPTURED launch needs: the device tensor is allocated once and only ever updated in place, rows are append-only (a captured
    launch bakes in the table's address and its row count: it keeps refreshing exactly the rows that existed when it was
    captured), and a row whose weights died is NEUTRALISED (source pointer 0: the kernel skips it) instead of removed - its pack
    buffer goes back to the allocator, and a replay must neither read the dead weights (their memory may be unmapped after
    empty_cache: a GPU fault) nor write the buffer.  The first version rebuilt the table tensor at every registration: the decode
    graphs of bench.py replayed a pack launch over a freed table (memory access fault at address 0x1e000, round 4)."""
    CAP = 4096

    def __init__(self, words):
        self.words, self.host, self.dev, self.n, self.dirty = words, None, None, 0, False
        self.event = self.stream = None
        self.rows = {}                     # key -> row index
        self.entries = {}                  # key -> entry dict (alive ones)

    def add(self, key, row, entry, device):
        if self.n >= self.CAP:
            return False
        if self.host is None:
            self.host = torch.zeros(self.CAP, self.words, dtype=torch.int64)
            self.dev = torch.zeros(self.CAP, self.words, dtype=torch.int64, device=device)
        self.host[self.n] = torch.tensor(row, dtype=torch.int64)
        self.rows[key], self.entries[key] = self.n, entry
        self.n += 1
        self.dirty = True
        return True

    def drop(self, key):
        self.host[self.rows.pop(key)].zero_()
        del self.entries[key]
        self.dirty = True

    def sweep(self, is_dead):
        """Neutralise the rows of dead entries (called before every refresh launch outside a capture)."""
        for k in [k for k, e in self.entries.items() if is_dead(k, e)]:
            self.drop(k)

    def upload(self):
        if self.dirty and self.dev is not None:
            self.dev.copy_(self.host, non_blocking=False)
            self.dirty = False

    def clear(self):
        """Forget every entry (test teardown); the device tensor stays (an old graph may still hold its address)."""
        for k in list(self.entries):
            self.drop(k)
        self.upload()
        self.event = self.stream = None


_ROW = _PackTable(6)        # rows: { W, packed, R, Cc, row stride, transposed }; key = (address, R, Cc, row stride, transposed)


def _row_dead(key, ent):
    """A _ROW row must not be refreshed again: its owner is gone, OR the owner lives on at another address (`p.data = view`:
    ParamArena, load_state_dict-style re-pointing) - the row's source address is then the freed old storage."""
    o = ent["owner"]()
    return o is None or o.data_ptr() + ent.get("off", 0) != key[0]


def _pack_done(tab):
    """The refresh launch sits on the current stream: remember it, consumers on OTHER streams (the right-to-left decoder, the CTC
    head) order themselves behind it."""
    ev = torch.cuda.Event()
    ev.record()
    tab.event, tab.stream = ev, torch.cuda.current_stream()


def _pack_wait(tab):
    if tab.event is not None and tab.stream != torch.cuda.current_stream():
        torch.cuda.current_stream().wait_event(tab.event)


def pack_events_forget():
    """planes.capture_scope() on exit: an event recorded INSIDE a capture must not be waited on by an eager consumer (every entry
    is stale after the scope - the generation moves - so the next eager reader refreshes and records a real event)."""
    for tab in (_ROW, _FFN):
        tab.event = tab.stream = None


def row_packs_clear():
    _ROW.clear()


def _row_pieces(k):
    return (k[1] // 32) * (k[2] // 16) if not k[4] else (k[2] // 32) * (k[1] // 16)


def _row_packed(w, transposed):
    """Packed fragments of Wg = w (x W^T) or w^T (dy W), fresh for the weight's current values; None if w cannot be registered."""
    owner = w._base if w._base is not None else w
    # only weights that OWN their memory for good: a Parameter (or a view of one), or a window of the parameter arena.  A temporary -
    # q / k / v weights concatenated for the fused projection of a model without an arena - dies after the call and the next
    # temporary lands on its address with other values and the same version: its cached pack would be taken for fresh
    a = _arena.active()
    if not (isinstance(owner, torch.nn.Parameter) or (a is not None and owner is a.flat)):
        return None
    key = (w.data_ptr(), w.shape[0], w.shape[1], w.stride(0), int(transposed))
    ent = _ROW.entries.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is not None and (ent["owner"]() is not owner or _row_dead(key, ent)):   # a new tenant: the old row dies, a new one is appended
        if capturing:
            return None
        _ROW.drop(key)
        ent = None
    if ent is None:
        if capturing:
            return None                                       # (its buffer would live in the graph's pool: stay on oe_gemm_f32)
        ent = dict(owner=weakref.ref(owner), off=key[0] - owner.data_ptr(), buf=torch.empty(w.shape[0] * w.shape[1] * 6, dtype=torch.uint8, device=w.device), gen=-1, ver=None)
        if not _ROW.add(key, [key[0], ent["buf"].data_ptr(), key[1], key[2], key[3], key[4]], ent, w.device):
            return None
    gen, ver = _planes.weights_generation(), owner._version
    if ent["gen"] != gen or ent["ver"] != ver:
        if not capturing:
            _ROW.sweep(_row_dead)
            _ROW.upload()
        elif _ROW.dirty:
            return None
        # every registered matrix in one launch (all of them are stale together: the generation moved)
        hip.call("oe_rowgemm6_pack_table", _ROW.dev, _ROW.n, max(_row_pieces(k) for k in _ROW.entries))
        _pack_done(_ROW)
        for e in _ROW.entries.values():
            o = e["owner"]()
            e["gen"], e["ver"] = gen, (None if o is None else o._version)
    else:
        _pack_wait(_ROW)
    return ent["buf"]


def _rowgemm_try(x, w, transposed, bias, out, epi, ln_pending=None, lnf_pending=None, ln_epi=None):
    """x (M, k) @ Wg^T on the row-block / tile kernels if the problem and its epilogue qualify; returns out or None.
    ln_pending: x is the `g` of a parked LayerNorm backward (_PENDING_LN) - launched as the kernel's prologue when this is the
    k = 256 row-block kernel, and on its own BEFORE anything reads x in every other case (also when None is returned)."""
    try:
        return _rowgemm_try_impl(x, w, transposed, bias, out, epi, ln_pending, lnf_pending, ln_epi)
    finally:
        if ln_pending is not None:
            ln_pending.resolve()                 # (no-op when the fused launch has happened)
        if lnf_pending is not None:
            lnf_pending.resolve()


def _rowgemm_try_impl(x, w, transposed, bias, out, epi, ln_pending, lnf_pending=None, ln_epi=None):
    if not ROWGEMM or hip.GEMM_PRECISION != 6 or not x.is_cuda:
        return None
    k = x.shape[1]
    n = w.shape[1] if transposed else w.shape[0]
    if (w.shape[0] if transposed else w.shape[1]) != k:
        return None
    form = hip.lib().oe_rowgemm6_form(x.shape[0], k, n)      # 2: tile form (few rows), 1: row-block form
    if form == 0 or (form == 1 and x.shape[0] < ROWGEMM_MIN_ROWS) or (form == 2 and not ROWTILE):
        return None
    ok = _ROW_EPI_OK if form == 1 else _ROWTILE_EPI_OK
    for key, v in epi.items():                                 # an epilogue feature the kernel does not have: oe_gemm_f32
        unset = v is None or (not isinstance(v, torch.Tensor) and (v is False or v == 0 or (key == "beta" and v == 1.0)))
        if not unset and key not in ok:
            return None
    act = epi.get("act", 0) or 0
    pre_out, aux_in, ld_aux = epi.get("preact_out"), epi.get("actgrad_in"), epi.get("ld_aux", 0) or 0
    if act not in (0, ACT_RELU, ACT_SWISH) or (pre_out is not None and aux_in is not None):
        return None
    for t in (pre_out, aux_in):
        if t is not None and (t.dtype != torch.float32 or t.data_ptr() % 8 or ld_aux % 2):
            return None
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16 or w.stride(1) != 1 or w.stride(0) % 4 or w.data_ptr() % 16:
        return None
    res = epi.get("residual")
    if res is not None and (res.stride(-1) != 1 or res.data_ptr() % 16 or epi.get("ldr", 0) % 4):
        return None
    if bias is not None and bias.data_ptr() % 16:
        return None
    wp = _row_packed(w, transposed)
    if wp is None:
        return None
    M = x.shape[0]
    if out is None:
        out = _new(M, n, like=x)
    elif out.stride(1) != 1 or out.stride(0) % 4 or out.data_ptr() % 16:
        return None
    global ROWGEMM_LAUNCHES
    ROWGEMM_LAUNCHES += 1
    ln = lnf = None
    if ln_pending is not None and not ln_pending.done:
        sd = epi.get("seed_dev")
        if (form == 1 and k == 256 and x.is_contiguous() and x.data_ptr() == ln_pending.g.data_ptr() and M == ln_pending.rows and
                (sd is None or _seed_dev is None or sd.data_ptr() == _seed_dev.data_ptr()) and (epi.get("drop_p", 0.0) or 0.0) == 0.0):
            ln = ln_pending.prologue()
        else:
            ln_pending.resolve()                # this launch reads x: the LayerNorm backward first, on its own
    if lnf_pending is not None and not lnf_pending.done:
        q = lnf_pending
        if form == 1 and k == 256 and ln is None and x.is_contiguous() and x.data_ptr() == q.y.data_ptr() and M == q.rows and q.gamma2 is None:
            lnf = q.prologue()
        else:
            q.resolve()                         # this launch reads x: the LayerNorm first, on its own
    lne = None
    if (ln_epi is not None and form == 1 and k == 256 and n == 256 and lnf is None and bias is None and not epi and
            M == ln_epi["dx"].shape[0] and ln_epi["dx"].is_contiguous() and ln_epi["x"].is_contiguous()):
        lne = ln_epi                            # the product leaves through a LayerNorm backward: `out` is not written, ln_epi["dx"] is
    hip.rowgemm6(x, wp, out, M, k, n, bias=bias, drop_p=epi.get("drop_p", 0.0) or 0.0, seed=epi.get("seed", 0) or 0,
                 seed_dev=(_seed_dev if ln is not None else epi.get("seed_dev")),
                 rowmask=epi.get("rowmask"), residual=res, ldr=epi.get("ldr", 0) or 0, beta=epi.get("beta", 1.0),
                 act=act, preact_out=pre_out, actgrad_in=aux_in, ld_aux=ld_aux, ln=ln, lnf=lnf, lne=lne)
    if lne is not None:
        ln_epi["done"] = True
    if ln is not None:
        ln_pending.fused()
    if lnf is not None:
        lnf_pending.fused()
    return out


def gemm_nt(x, w, bias=None, out=None, out_planes=False, **epi):
    """y[M,N] = x[M,K] @ w[N,K]^T (+ epilogue).  out_planes: the output is a later GEMM's operand - write its bf16 planes too."""
    M, K = x.shape
    N = w.shape[0]
    lnf = _PENDING_LNF.take(x)                                                    # x may be the output of a parked LayerNorm forward
    if not (out_planes and _planes.split_activations()):
        y = _rowgemm_try(x, w, False, bias, out, epi, lnf_pending=lnf)             # (launches or resolves it on every path)
        if y is not None:
            return y
    elif lnf is not None:
        lnf.resolve()
    if out is None:
        out = _new(M, N, like=x)
    ap, bp = _operand_planes(x, w)
    cp = _planes.new_output(out) if (out_planes and _planes.split_activations() and out.numel() >= _planes.MIN_SPLIT_ELEMS) else None
    hip.gemm(x, w, out, M, N, K, lda=x.stride(0), ldb=w.stride(0), ldc=out.stride(0), bias=bias, a_planes=ap, b_planes=bp, c_planes=cp, **epi)
    return out


def gemm_nn(dy, w, out=None, out_planes=False, ln_epi=None, **epi):
    """dx[M,K] = dy[M,N] @ w[N,K].  out_planes: True = with the general pre-split policy, "always" = whenever pre-split
    operands exist at all (the conv front end's policy)."""
    M, N = dy.shape
    K = w.shape[1]
    pend = _PENDING_LN.take(dy)                                                   # dy is the g of a parked LayerNorm backward
    if not (out_planes and (_planes.available() if out_planes == "always" else _planes.split_activations())):
        y = _rowgemm_try(dy, w, True, None, out, epi, ln_pending=pend, ln_epi=ln_epi)      # (launches or resolves it on every path)
        if y is not None:
            return y
    elif pend is not None:
        pend.resolve()
    if out is None:
        out = _new(M, K, like=dy)
    ap, bp = _operand_planes(dy, w)
    want = _planes.available() if out_planes == "always" else (out_planes and _planes.split_activations())
    cp = _planes.new_output(out) if (want and out.numel() >= _planes.MIN_SPLIT_ELEMS) else None
    hip.gemm(dy, w, out, M, K, N, lda=dy.stride(0), ldb=w.stride(0), ldc=out.stride(0), b_kmajor=True, a_planes=ap, b_planes=bp, c_planes=cp, **epi)
    return out


def gemm_nn_deep(dy, w, alpha_dev=None):
    """dx[M,K] = dy[M,N] @ w[N,K] for a deep reduction into a narrow output (the activation gradient through a vocabulary
    projection: N = 3246, K = 256).  One 64x64 tile per block walks the whole reduction: with few tiles the chip is mostly
    idle and the launch is bound by the latency of ~100 dependent K-tiles.  Split-K with atomic accumulation into a zeroed
    output puts ~2000 blocks in flight (tools/deepk_scan.py: 992 rows 138 -> 27.5 us at 8 splits, 7936 rows 163 -> 94 us
    at 4; odd split counts measured slower)."""
    M, N = dy.shape
    K = w.shape[1]
    tiles = -(-M // 64) * -(-K // 64)
    sk = 1
    if hip.GEMM_PRECISION != 0 and N >= 2048 and K <= 512:
        want = -(-1984 // tiles)
        sk = 8 if want >= 8 else 4 if want >= 3 else 2
    if sk == 1:
        return gemm_nn(dy, w, alpha_dev=alpha_dev)
    out = _new(M, K, like=dy, zero=True)
    hip.gemm(dy, w, out, M, K, N, lda=dy.stride(0), ldb=w.stride(0), ldc=out.stride(0), b_kmajor=True, split_k=sk,
             atomic_out=True, alpha_dev=alpha_dev)
    return out


def wgrad_planes(dy, x, always=False):
    """Pre-split copies of both operands of a weight gradient dy^T x (both activations), or (None, None).
    always: under the conv front end's policy too (not only the general one)."""
    if not (_planes.available() if always else _planes.active()):
        return None, None
    make = always or _planes.split_activations()
    ap = _planes.of(dy, make=make)
    bp = _planes.of(x, make=make) if ap is not None else None
    return (ap, bp) if bp is not None else (None, None)


def gemm_tn(dy, x, out=None, alpha=1.0, alpha_dev=None, bias_out=None, planes=None):
    """dw[N,K] (+)= dy[M,N]^T @ x[M,K]  (split-K, atomic accumulation into `out`).
    bias_out (optional, [N], accumulated): alpha * column sums of dy - fused into the GEMM on the
    bf16 paths, a separate column-sum launch on the exact-fp32 path.
    planes: (dy planes, x planes) resolved by the caller (deferred launches resolve them when the gradient is requested)."""
    M, N = dy.shape
    K = x.shape[1]
    if out is None:
        out = _new(N, K, like=dy, zero=True)
    fused = bias_out is not None and hip.GEMM_PRECISION != 0
    ap, bp = planes if planes is not None else wgrad_planes(dy, x)
    hip.gemm(dy, x, out, N, K, M, lda=dy.stride(0), ldb=x.stride(0), ldc=out.stride(0), a_kmajor=True, b_kmajor=True,
             split_k=_split_k(N, K, M), atomic_out=True, alpha=alpha, alpha_dev=alpha_dev,
             a_colsum=bias_out if fused else None, a_planes=ap, b_planes=bp)
    if bias_out is not None and not fused:
        colsum(dy, alpha, alpha_dev, N, out=bias_out)
    return out


def colsum(x, alpha=1.0, alpha_dev=None, n=None, out=None):
    M = x.shape[0]
    n = x.shape[1] if n is None else n
    acc = out is not None
    if out is None:
        out = _new(n, like=x)
    hip.call("oe_colsum_f32", x, x.stride(0), M, n, alpha, alpha_dev, out, int(acc))
    return out


# ---- weight-gradient GEMMs on a side stream -----------------------------------
# Nothing downstream of backward consumes a parameter gradient before the optimizer, so (with a
# ParamArena as the destination) the wgrad GEMMs can run on a second HIP stream beside the
# activation-gradient chain and fill its bubbles.  The engine joins the streams after backward.
ASYNC_WGRAD = False
_side_stream = None


def side_stream():
    global _side_stream
    if _side_stream is None:
        _side_stream = torch.cuda.Stream()
    return _side_stream


# ---- phase stamps (diagnostic, tools/phase_stamps.py): STAMPS = {"buf": int64 device tensor, "tags": [...]} or None ----------
STAMPS = None


def stamp(tag: str):
    """Record the wall clock when the current stream gets here (no-op unless a tool switched STAMPS on)."""
    if STAMPS is None:
        return
    slot = len(STAMPS["tags"])
    if slot >= STAMPS["buf"].numel():
        return
    STAMPS["tags"].append(tag)
    hip.call("oe_stamp", STAMPS["buf"], slot)


def stamp_grad(x: torch.Tensor, tag: str) -> None:
    """Stamp when backward has produced the gradient of x."""
    if STAMPS is not None and x.requires_grad:
        x.register_hook(lambda g, tag=tag: stamp(tag))


# ---- cut points for a step captured in segments (TrainEngine.capture with several ranks) ---------------------------------
# At a cut the forward value passes through unchanged, but the autograd tape is severed: the engine first differentiates
# from the loss down to the last cut (its gradient lands in `leaf.grad`), then resumes from each cut's upstream side
# with that gradient - one HIP graph per piece, a gradient all-reduce issued between the replays.
CUTS = None          # None: cut() is the identity.  A list: (name, upstream tensor, leaf) per cut, in forward order.


def cut(x: torch.Tensor, name: str) -> torch.Tensor:
    if CUTS is None or not x.requires_grad:
        return x
    leaf = x.detach().requires_grad_(True)
    CUTS.append((name, x, leaf))
    return leaf


def forked_streams():
    """Every stream the step may fork work onto (the engine checks that a capture has led them all back)."""
    return [s for s in (_side_stream, _decoder_stream, _ctc_stream) if s is not None] + list(_extra_streams)


_extra_streams = []          # streams registered by callers that fork on their own (tests; experiments)


def join_side_stream():
    flush_wgrads()
    if _side_stream is not None:
        torch.cuda.current_stream().wait_stream(_side_stream)
    if _decoder_stream is not None:
        torch.cuda.current_stream().wait_stream(_decoder_stream)
    if _ctc_stream is not None:
        torch.cuda.current_stream().wait_stream(_ctc_stream)


# ---- the right-to-left decoder beside the left-to-right one -----------------------
# The two decoders of the bi-decoder (decoder.py:278-309) share nothing but their inputs, and their launches are small
# (992 rows: 16 x 4 tiles of a GEMM, i.e. 64 blocks on 256 CUs, each bound by its own latency).  With this switch on,
# ASRModel._calc_att_loss runs the right decoder and its loss head on a second stream: ONE fork after the encoder, ONE
# join where the two losses are combined; autograd replays each node on the stream of its forward, so backward forks
# the same way.  (The per-layer weight-gradient fork above is a different matter: hundreds of cross-queue waits.)
PARALLEL_DECODERS = False
_decoder_stream = None


_ctc_stream = None


def ctc_stream():
    global _ctc_stream
    if _ctc_stream is None:
        _ctc_stream = torch.cuda.Stream()
    return _ctc_stream


def decoder_stream():
    global _decoder_stream
    if _decoder_stream is None:
        _decoder_stream = torch.cuda.Stream()
    return _decoder_stream


class _Side:
    """Run the enclosed launches on the side stream, ordered after everything enqueued so far."""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if isinstance(t, torch.Tensor)]

    def __enter__(self):
        side = side_stream()
        side.wait_stream(torch.cuda.current_stream())
        self.cm = torch.cuda.stream(side)
        self.cm.__enter__()

    def __exit__(self, *exc):
        self.cm.__exit__(*exc)
        for t in self.tensors:                 # keep the allocator from recycling inputs the side stream still reads
            t.record_stream(_side_stream)
        return False


class _Inline:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def _wgrad_ctx(to_arena: bool, *tensors):
    return _Side(*tensors) if (ASYNC_WGRAD and to_arena) else _Inline()


# Deferred form for captured graphs: a cross-queue edge costs ~6 us at replay, so a fork per weight gradient (150 of them)
# loses more than the overlap gives (21.5 vs 19.6 ms/step).  With WGRAD_DEFER = n > 0 the launches are collected instead
# (the closures keep their operands alive) and every n of them go to the side stream behind ONE fork; the engine flushes
# the rest and joins after backward.  Operands are never modified in place after a weight gradient has been requested
# (the eager side stream relies on the same property).
WGRAD_DEFER = 0
_deferred = []


def _run_wgrad(to_arena: bool, tensors, fn, desc=None):
    """desc (optional): the launch as data - dict(dy, x, out, alpha, alpha_dev, bias_out) of a plain `out += alpha dy^T x` -
    so that a flush can run the small ones of a group as ONE grouped launch (WGRAD_GROUPED)."""
    if WGRAD_DEFER > 0 and to_arena:
        # the stream that produces this launch's operands: the flush must order the side stream after every one of them
        # (the decoders' backward runs on other streams than the encoder's)
        _deferred.append((fn, [t for t in tensors if isinstance(t, torch.Tensor)], torch.cuda.current_stream(), desc))
        if len(_deferred) >= WGRAD_DEFER:
            flush_wgrads()
        return
    with _wgrad_ctx(to_arena, *tensors):
        fn()


# The weight gradients of a flush as ONE launch of the bf16-planes kernel (oe_gemm_tn_grouped).  Alone each output of a few
# 128 x 128 tiles over K = B T' rows needs a 16-60-way split of the reduction to cover the chip and spends much of its time
# in the atomic epilogue (the four small ones of an encoder layer: 81 us one by one, 41 us together).  Measured in the step
# (one box, repeated): everything up to 12 tiles grouped 15.34 ms/step, up to 16 / 24 / 48 tiles 15.40 / 15.47 / 15.34-15.49,
# nothing grouped 15.86 - the feed-forward's 16-tile outputs fill the chip on their own and the 52-tile vocabulary
# projections (other reduction lengths) unbalance a group.
WGRAD_GROUPED = os.environ.get("OE_WGRAD_GROUPED", "1") == "1"
WGRAD_GROUP_MAX_TILES = int(os.environ.get("OE_WGRAD_GROUP_MAX_TILES", "12"))     # outputs of more tiles than this are launched on their own
WGRAD_GROUP_BLOCKS = int(os.environ.get("OE_WGRAD_GROUP_BLOCKS", "512"))           # blocks a grouped launch aims for (sets the split of the reductions)
_TN_TABLES = []                    # eager flushes: (device table, host bytes) kept until the stream has surely consumed them


def _group_wgrads(descs):
    """Launch the groupable ones among `descs` (current stream = the side stream); returns the set of indices it covered."""
    if hip.GEMM_PRECISION == 0:
        return set()
    idx = []
    for i, d in enumerate(descs):
        if d is None:
            continue
        dy, x, out = d["dy"], d["x"], d["out"]
        tiles = -(-dy.shape[1] // 128) * -(-x.shape[1] // 128)
        ok = (dy.dim() == 2 and x.dim() == 2 and out.dim() == 2 and dy.stride(1) == 1 and x.stride(1) == 1 and out.stride(1) == 1 and
              dy.shape[0] == x.shape[0] and dy.shape[0] >= 128 and tiles <= WGRAD_GROUP_MAX_TILES and dy.shape[1] >= 4 and x.shape[1] >= 4 and
              dy.stride(0) % 4 == 0 and x.stride(0) % 4 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and
              dy.stride(0) >= -(-dy.shape[1] // 4) * 4 and x.stride(0) >= -(-x.shape[1] // 4) * 4)
        if ok:
            idx.append(i)
    if len(idx) < 2:
        return set()
    plan = hip.tn_grouped_plan([descs[i] for i in idx], WGRAD_GROUP_BLOCKS)
    if plan is None:
        return set()
    host, total = plan
    table = torch.empty(len(host), dtype=torch.uint8, device=descs[idx[0]]["dy"].device)
    if LN_TABLE is not None and not LN_TABLE.eager:
        LN_TABLE.uploads.append((table, host))                         # inside a capture: filled by ln_table_end, kept with the graph
    else:
        # stream-ordered upload from pinned memory: the host never waits for the stream (bench.py's bracketed steps park the GPU
        # while the host enqueues the whole step)
        pinned = torch.frombuffer(bytearray(host), dtype=torch.uint8).pin_memory()
        table.copy_(pinned, non_blocking=True)
        _TN_TABLES.append((table, pinned))
        del _TN_TABLES[:-64]
    hip.tn_grouped_launch(table, len(idx), total,
                          flops=sum(2.0 * descs[i]["dy"].shape[0] * descs[i]["dy"].shape[1] * descs[i]["x"].shape[1] for i in idx))
    return set(idx)


def drop_deferred():
    """Forget deferred launches without running them (after a failed capture)."""
    global _deferred
    _deferred = []


# Measurement aid (bench.py's event-bracketed steps, `--single-stream` profile runs): run a flush on the CURRENT stream, so that
# an eager step launches exactly the kernels a captured step holds - the grouped weight gradients included - one after the other.
WGRAD_FLUSH_INLINE = False


def flush_wgrads():
    global _deferred
    if not _deferred:
        return
    if WGRAD_FLUSH_INLINE:
        grouped = _group_wgrads([d for _, _, _, d in _deferred]) if WGRAD_GROUPED else set()
        for i, (fn, _, _, _) in enumerate(_deferred):
            if i not in grouped:
                fn()
        _deferred = []
        return
    side = side_stream()
    origins = []
    for _, _, st, _ in _deferred:
        if all(st != o for o in origins):
            origins.append(st)
    for st in origins:
        side.wait_stream(st)
    with torch.cuda.stream(side):
        grouped = _group_wgrads([d for _, _, _, d in _deferred]) if WGRAD_GROUPED else set()
        for i, (fn, _, _, _) in enumerate(_deferred):
            if i not in grouped:
                fn()
    for _, ts, _, _ in _deferred:
        for t in ts:
            t.record_stream(side)
    _deferred = []


# ---- parameter-gradient sinks ------------------------------------------------
# With a ParamArena active the kernels accumulate into the flat gradient buffer and
# autograd is told "no gradient" (None); otherwise a fresh tensor is returned.
def wgrad(param, dy, x, alpha=1.0, alpha_dev=None):
    tgt = _arena.grad_target(param)
    if tgt is None:
        return gemm_tn(dy, x, alpha=alpha, alpha_dev=alpha_dev).view(param.shape)
    out = tgt.view(dy.shape[1], x.shape[1])
    pl = wgrad_planes(dy, x)
    _run_wgrad(True, (dy, x, alpha_dev) + _pl_tensors(pl), lambda: gemm_tn(dy, x, out=out, alpha=alpha, alpha_dev=alpha_dev, planes=pl),
               desc=dict(dy=dy, x=x, out=out, alpha=alpha, alpha_dev=alpha_dev, bias_out=None))
    return None


def _pl_tensors(pl):
    """The bf16 tensors behind a (dy planes, x planes) pair, for stream bookkeeping."""
    return tuple(q.t for q in pl if q is not None) if pl is not None else ()


def _sink_swapped(param, src, A, Bd, Cd):
    """param-grad = swap_last2(src viewed [A][Bd][Cd]) accumulated into the arena or returned."""
    tgt = _arena.grad_target(param)
    if tgt is None:
        out = torch.empty_like(param)
        hip.call("oe_swap_last2", src, A, Bd, Cd, out, 0)
        return out
    hip.call("oe_swap_last2", src, A, Bd, Cd, tgt, 1)
    return None


def wgrad_bias(w, b, dy, x, alpha=1.0, alpha_dev=None):
    """Weight and bias gradient of y = x w^T + b from dy in ONE GEMM launch (bias = fused column sums).
    Returns what autograd should see: (dw, db), each None when it went straight into the arena."""
    if b is None:
        return wgrad(w, dy, x, alpha, alpha_dev), None
    N, K = dy.shape[1], x.shape[1]
    tw, tb = _arena.grad_target(w), _arena.grad_target(b)
    ow = tw.view(N, K) if tw is not None else _new(N, K, like=dy, zero=True)
    ob = tb if tb is not None else _new(N, like=dy, zero=True)
    pl = wgrad_planes(dy, x)
    _run_wgrad(tw is not None and tb is not None, (dy, x, alpha_dev) + _pl_tensors(pl),
               lambda: gemm_tn(dy, x, out=ow, alpha=alpha, alpha_dev=alpha_dev, bias_out=ob, planes=pl),
               desc=dict(dy=dy, x=x, out=ow, alpha=alpha, alpha_dev=alpha_dev, bias_out=ob))
    return (None if tw is not None else ow.view(w.shape)), (None if tb is not None else ob)


def bgrad(param, dy, alpha=1.0, alpha_dev=None, n=None):
    if param is None:
        return None
    tgt = _arena.grad_target(param)
    if tgt is None:
        return colsum(dy, alpha, alpha_dev, n)
    colsum(dy, alpha, alpha_dev, n, out=tgt)
    return None


def grad_sink(param):
    """(buffer the kernel accumulates into, value to hand back to autograd)."""
    tgt = _arena.grad_target(param)
    if tgt is None:
        z = torch.zeros_like(param)
        return z, z
    return tgt.view(param.shape), None


def _fused_rows(parts, cat_dim0=True):
    """Weights that sit back to back in the arena are used in place; otherwise concatenated."""
    a = _arena.active()
    if a is not None and a.enabled and a.adjacent(*parts):
        rows = sum(p.shape[0] for p in parts)
        return torch.as_strided(parts[0], (rows,) + tuple(parts[0].shape[1:]), parts[0].stride()), True
    return torch.cat(list(parts), 0), False


def dropout_scale(x, alpha=1.0, p=0.0, seed=0, rowmask=None, cols=None):
    out = torch.empty_like(x)
    cols = x.shape[-1] if cols is None else cols
    hip.call("oe_dropout_scale", x, x.numel(), cols, alpha, p, seed, _seed_dev, rowmask, out)
    return out


# --------------------------------------------------------------------------- #
# LayerNorm
# --------------------------------------------------------------------------- #
def _ln_ws(like, rows, d):
    return _new(hip.lib().oe_layernorm_bwd_workspace_floats(rows, d), like=like)


def _ln_fwd(x, gamma, beta, eps, rows, d, rowmask, act, y, stats, planes_out=True):
    """LayerNorm forward; in the pre-split mode the output also leaves as bf16 planes (it feeds a GEMM)."""
    pl = _planes.new_output(y.view(rows, d)) if (planes_out and _planes.active() and rows * d >= _planes.MIN_SPLIT_ELEMS) else None
    if pl is None:
        hip.call("oe_layernorm_fwd", x, gamma, beta, eps, rows, d, rowmask, act, y, stats)
    else:
        hip.call("oe_layernorm_fwd_pl", x, gamma, beta, eps, rows, d, rowmask, act, y, stats, pl.t, pl.stride)


# While a training step is being captured into a HIP graph, LayerNorm backward leaves the reduction of its per-block
# parameter-gradient partials to ONE table-driven launch at the end of backward (ln_table_flush) instead of one small
# launch per call.  The table is a device tensor allocated before the capture; the host fills it after the capture (the
# workspaces' addresses inside the graph's memory pool are the same at every replay).
LN_TABLE_CAPACITY = 512


class _LnTable:
    """The reduce table of one step: rows (workspace, rows, d, dgamma, dbeta) of oe_layernorm_param_reduce_table; keep: the
    workspaces of the rows since the last flush; uploads: (device table, host bytes) of grouped weight-gradient launches (_group_wgrads)."""
    __slots__ = ("dev", "eager", "entries", "keep", "max_rows", "max_d", "launched", "uploads")

    def __init__(self, dev, eager):
        self.dev, self.eager, self.entries, self.keep, self.uploads = dev, eager, [], [], []
        self.max_rows, self.max_d, self.launched = 1, 4, 0

    def add(self, ws, rows, d, dg, db):
        self.entries.append((ws.data_ptr(), rows, d, dg.data_ptr(), db.data_ptr()))
        self.keep.append(ws)
        self.max_rows, self.max_d = max(self.max_rows, rows), max(self.max_d, d)


LN_TABLE = None             # an _LnTable in table mode
LN_EAGER_TABLE = os.environ.get("OE_LN_EAGER_TABLE", "1") == "1"
_LN_EAGER_DEV = {}          # device -> the eager table's device tensor (allocated once)
_LN_EAGER_PINNED = []       # pinned host tables of the last flushes (alive until their stream-ordered uploads have surely run)


def ln_table_begin(device, eager=False):
    """eager: table mode for an eager step too (TrainEngine) - the table is uploaded stream-ordered right before the launch that reads it
    (a captured step fills it once after the capture, ln_table_end)."""
    global LN_TABLE
    if eager:
        dev = _LN_EAGER_DEV.get(device)
        if dev is None:
            dev = _LN_EAGER_DEV[device] = torch.zeros(LN_TABLE_CAPACITY, 5, dtype=torch.int64, device=device)
    else:
        dev = torch.zeros(LN_TABLE_CAPACITY, 5, dtype=torch.int64, device=device)
    LN_TABLE = _LnTable(dev, eager)
    return LN_TABLE


def ln_table_flush():
    """Enqueue the reduction of everything recorded since the last flush (current stream; call after the side streams
    have been joined)."""
    t = LN_TABLE
    if t is None or len(t.entries) == t.launched:
        return
    first, n = t.launched, len(t.entries) - t.launched
    assert len(t.entries) <= LN_TABLE_CAPACITY, "LN_TABLE_CAPACITY exceeded"
    if t.eager:
        host = torch.tensor(t.entries[first:], dtype=torch.int64).pin_memory()
        t.dev[first:first + n].copy_(host, non_blocking=True)
        _LN_EAGER_PINNED.append(host)
        del _LN_EAGER_PINNED[:-8]
        cur = torch.cuda.current_stream()
        for ws in t.keep:
            ws.record_stream(cur)               # (workspaces of norms that ran on the decoders' streams)
    hip.call("oe_layernorm_param_reduce_table", t.dev[first:], n, t.max_rows, t.max_d)
    t.launched = len(t.entries)
    t.keep = []                         # later allocations may reuse the workspaces: they come after this launch in stream order


def ln_table_end():
    """After the capture: upload the table (host -> device copy, not capturable) and leave table mode."""
    global LN_TABLE
    t, LN_TABLE = LN_TABLE, None
    if t is not None and t.entries:
        t.dev[: len(t.entries)].copy_(torch.tensor(t.entries, dtype=torch.int64))
    if t is not None:
        for table, host in t.uploads:           # grouped weight-gradient tables recorded during the capture
            table.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
    return t


def _ln_param_reduce(ws, rows, d, dg, db, to_arena):
    """A LayerNorm backward's parameter-gradient partials: a row of the active table (arena gradients only), or a reduce launch now."""
    if LN_TABLE is not None and to_arena:
        LN_TABLE.add(ws, rows, d, dg, db)
    else:
        hip.call("oe_layernorm_param_reduce", ws, rows, d, dg, db)


# A block's output is `residual + out_scale * dropout(f(LN(x)))`, and the LayerNorm that consumes it belongs to the NEXT block:
# in backward that LayerNorm's dx is exactly the gradient the block starts from, which it first multiplies by its output
# dropout mask and scale.  The block tags its output (FUSE_OUT_DROP); the next LayerNorm backward then writes that product
# as a second output of its kernel (oe_layernorm_bwd_dx_drop) and the block's backward picks it up by the address of the
# gradient it receives - one elementwise launch per block (66 per step at config 2) less.  Anything in between (an adapter's
# add, a gradient autograd had to accumulate) changes the address and the block falls back to oe_dropout_scale.
# Entries live from the LayerNorm backward that makes them to the block backward that consumes them; whatever is left
# (a block that was never differentiated) is dropped when the next forward pass starts (ASRModel.forward /
# LanguageModel.forward / TrainEngine call predrop_clear).
FUSE_OUT_DROP = os.environ.get("OE_FUSE_OUT_DROP", "1") == "1"
_PREDROP = {}


def predrop_clear():
    """Called where a new step starts (ASRModel.forward / LanguageModel.forward / TrainEngine): drops the previous step's
    leftovers - dropped-gradient copies and the registry of pre-split GEMM operands."""
    resolve_pending_ln()
    resolve_pending_lnf()
    _PREDROP.clear()
    _planes.clear()


def _tag_out_drop(out, out_scale, p_out, s_out, rowmask=None, ln_fuse=False):
    if FUSE_OUT_DROP and (p_out > 0 or out_scale != 1.0 or rowmask is not None):
        out._oe_outdrop = (float(out_scale), float(p_out), int(s_out), rowmask)
        if ln_fuse:
            out._oe_lnfuse = True          # this block's backward can take the next LayerNorm's backward into its first GEMM (_ln_bwd)
    return out


# The LayerNorm backward in front of a block's backward as the PROLOGUE of that block's first input-gradient GEMM (oe_rowgemm6's
# ln_* arguments): the block (attention: linear_out; conv module: pointwise_conv2) says at forward time that its backward starts with
# `g = _out_drop_grad(dy)` followed by `gemm_nn(g, w)` on the row-block kernel (_ln_fuse_ok); the pre-norm fork that consumes the
# block's output then does NOT launch its backward kernel but parks its arguments here, keyed by the address of g; gemm_nn finds
# them and launches the fused kernel, which writes dx and g before anything else can read them.  Every other path out of
# _out_drop_grad / gemm_nn resolves a parked entry by launching the LayerNorm backward on its own (_LnBwdPark.resolve), and
# TrainEngine checks that none is left behind.  24 launches per step at config 2 (10.8 us + a dependent-launch gap each).
LN_BWD_FUSE = os.environ.get("OE_LN_BWD_FUSE", "1") == "1"
LN_BWD_FUSED_LAUNCHES = 0       # (tests)
LN_EPI_FUSE = os.environ.get("OE_LN_EPI_FUSE", "1") == "1"      # the conv module's norm backward as an epilogue (ConvModuleFn.backward)
LN_EPI_FUSED_LAUNCHES = 0
_PENDING_LN = _ParkRegistry("g")


def resolve_pending_ln():
    """Safety net (TrainEngine after backward, predrop_clear): a parked LayerNorm backward nobody picked up.  Returns the count."""
    return _PENDING_LN.sweep()


def _ln_rows_fusable(rows, d):
    """Rows the k = 256 row-block kernels can make with a LayerNorm prologue / epilogue (each site adds its switches and conditions)."""
    return hip.GEMM_PRECISION == 6 and d == 256 and rows >= ROWGEMM_MIN_ROWS and not _planes.active()


def _ln_fuse_ok(rows, d, w):
    """Forward-time promise of a block whose backward starts with gemm_nn(g, w), w (d, d): will that be the k = 256 row-block kernel?"""
    return LN_BWD_FUSE and ROWGEMM and FUSE_OUT_DROP and _ln_rows_fusable(rows, d) and w.shape[0] == 256 and w.shape[1] == 256


class _LnBwdPark:
    """A parked LayerNorm backward (_ln_bwd), or the pair form (NormPairFn.backward: LN1 with beta, LN2 with gamma2 / stats2 / ws2).
    Its parameter-gradient partials become rows of LN_TABLE if one is active when it is parked (made: the rows belong to the
    ln_table_flush that follows the norm's own backward, wherever it is launched), else they are reduced when it is launched."""
    __slots__ = ("dy", "x", "gamma", "beta", "stats", "add", "dx", "g", "ws", "spec", "rows", "d", "dg", "db", "rowmask",
                 "gamma2", "stats2", "ws2", "dg2", "db2", "table", "done")

    def __init__(self, dy, x, gamma, beta, stats, add, dx, g, ws, spec, rows, d, dg, db, rowmask=None,
                 gamma2=None, stats2=None, ws2=None, dg2=None, db2=None):
        self.dy, self.x, self.gamma, self.beta, self.stats, self.add, self.dx, self.g = dy, x, gamma, beta, stats, add, dx, g
        self.ws, self.spec, self.rows, self.d, self.dg, self.db, self.rowmask = ws, spec, rows, d, dg, db, rowmask
        self.gamma2, self.stats2, self.ws2, self.dg2, self.db2 = gamma2, stats2, ws2, dg2, db2
        self.table, self.done = LN_TABLE is not None, False
        if self.table:
            for args in self._partials():
                LN_TABLE.add(*args)

    def _partials(self):
        one = (self.ws, self.rows, self.d, self.dg, self.db)
        return (one,) if self.gamma2 is None else (one, (self.ws2, self.rows, self.d, self.dg2, self.db2))

    def _launched(self):
        self.done = True
        if not self.table:
            for args in self._partials():
                hip.call("oe_layernorm_param_reduce", *args)

    def resolve(self):
        """The LayerNorm backward as a launch of its own (exactly what _ln_bwd / NormPairFn.backward would have launched)."""
        if self.done:
            return
        alpha, p, seed, gmask = self.spec
        if self.gamma2 is not None:
            hip.call("oe_layernorm_pair_bwd_dx_drop", self.dy, self.x, self.gamma, self.beta, self.stats, self.gamma2, self.stats2,
                     self.rows, self.d, self.add, self.dx, self.g, alpha, p, seed, _seed_dev, gmask, self.ws, self.ws2)
        else:
            hip.call("oe_layernorm_bwd_dx_drop", self.dy, self.x, self.gamma, self.beta, 0, self.stats, self.rows, self.d,
                     self.rowmask, self.add, self.dx, self.g, alpha, p, seed, _seed_dev, gmask, self.ws)
        self._launched()

    def prologue(self):
        """The `ln` argument of hip.rowgemm6 / hip.ffn_bwd (LnPrologue.fill)."""
        alpha, p, seed, gmask = self.spec
        return dict(dy=self.dy, x=self.x, stats=self.stats, gamma=self.gamma, add=self.add, dx=self.dx, g=self.g, ws=self.ws,
                    alpha=alpha, p=p, seed=seed, rowmask=gmask, ln_rowmask=self.rowmask, beta=self.beta if self.gamma2 is not None else None,
                    gamma2=self.gamma2, stats2=self.stats2, ws2=self.ws2)

    def fused(self):
        global LN_BWD_FUSED_LAUNCHES
        LN_BWD_FUSED_LAUNCHES += 1
        self._launched()


def _out_drop_grad(dy2, out_scale, p_out, s_out, rowmask=None):
    """dropout_scale(dy2, out_scale, p_out, s_out, rowmask) - or the copy the producing LayerNorm backward already made."""
    hit = _PREDROP.pop(dy2.data_ptr(), None)
    if hit is not None:
        # the entry keeps the producing dx alive, so no other tensor can have been given this address meanwhile; an
        # in-place change of dx since (autograd summing a second consumer's gradient into it) shows in its version
        g, spec, dx, version = hit
        same_mask = (spec[3] is None and rowmask is None) or (spec[3] is not None and rowmask is not None and
                                                               spec[3].data_ptr() == rowmask.data_ptr())
        if (dx._version == version and dx.numel() == dy2.numel() and spec[:3] == (float(out_scale), float(p_out), int(s_out)) and
                same_mask and g.numel() == dy2.numel()):
            return g.view(dy2.shape)              # (possibly still parked: the caller's gemm_nn comes next and launches it)
        pend = _PENDING_LN.take(g)
        if pend is not None:
            pend.resolve()
    return dropout_scale(dy2, out_scale, p_out, s_out, rowmask)


def _ln_bwd(dy, x, gamma, beta, act, stats, rows, d, rowmask, add, dx, dg, db, to_arena, prev_drop=None, fuse=False):
    ws = _ln_ws(x, rows, d)
    # (to_arena: the parameter gradients are written later than this function returns - fine for arena slices, which autograd never
    # sees, wrong for fresh tensors that PreNormFn.backward hands back to autograd right away)
    if (fuse and to_arena and prev_drop is not None and LN_BWD_FUSE and FUSE_OUT_DROP and act == ACT_NONE and _ln_rows_fusable(rows, d) and
            dy.is_contiguous() and x.is_contiguous() and (add is None or add.is_contiguous())):
        # parked: the consuming block's first input-gradient GEMM launches it as its prologue (see _PENDING_LN)
        g = torch.empty_like(dx)
        _PENDING_LN.park(_LnBwdPark(dy, x, gamma, beta, stats, add, dx, g, ws, prev_drop, rows, d, dg, db, rowmask=rowmask))
        _PREDROP[dx.data_ptr()] = (g, prev_drop, dx, dx._version)
        return
    if prev_drop is not None and FUSE_OUT_DROP and d % 8 == 0:
        g = torch.empty_like(dx)
        alpha, p, seed, gmask = prev_drop
        # g is what the previous block's backward GEMMs read: in the pre-split mode it leaves as bf16 planes too
        pl = _planes.new_output(g.view(rows, d)) if (_planes.active() and rows * d >= _planes.MIN_SPLIT_ELEMS) else None
        if pl is None:
            hip.call("oe_layernorm_bwd_dx_drop", dy, x, gamma, beta, act, stats, rows, d, rowmask, add, dx, g, alpha, p, seed, _seed_dev,
                     gmask, ws)
        else:
            hip.call("oe_layernorm_bwd_dx_drop_pl", dy, x, gamma, beta, act, stats, rows, d, rowmask, add, dx, g, alpha, p, seed, _seed_dev,
                     gmask, ws, pl.t, pl.stride)
        _PREDROP[dx.data_ptr()] = (g, prev_drop, dx, dx._version)
    else:
        hip.call("oe_layernorm_bwd_dx", dy, x, gamma, beta, act, stats, rows, d, rowmask, add, dx, ws)
    _ln_param_reduce(ws, rows, d, dg, db, to_arena)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, rowmask, act, sole_consumer=False):
        x = _chk(x, "layer_norm")
        d = x.shape[-1]
        rows = x.numel() // d
        y = torch.empty_like(x)
        stats = _new(rows, 2, like=x)
        _ln_fwd(x, gamma, beta, eps, rows, d, rowmask, act, y, stats)
        ctx.save_for_backward(x, gamma, beta, stats, rowmask)
        ctx.act = act
        # only when the caller vouches that x feeds nothing else: with a second consumer autograd SUMS the gradients of x
        # (possibly in place, keeping the address), and the fused copy would hold this branch's share only
        ctx.prev_drop = getattr(x, "_oe_outdrop", None) if sole_consumer else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats, rowmask = ctx.saved_tensors
        dy = dy.contiguous()
        d = x.shape[-1]
        rows = x.numel() // d
        dx = torch.empty_like(x)
        (dg, rg), (db, rb) = grad_sink(gamma), grad_sink(beta)
        _ln_bwd(dy, x, gamma, beta, ctx.act, stats, rows, d, rowmask, None, dx, dg, db, rg is None and rb is None, ctx.prev_drop)
        return dx, rg, rb, None, None, None, None


def layer_norm(x, gamma, beta, eps, rowmask=None, act=ACT_NONE, sole_consumer=False):
    """sole_consumer: x is used by nothing but this norm (lets backward hand the previous block its output-dropout gradient)."""
    return LayerNormFn.apply(x, gamma, beta, eps, rowmask, act, sole_consumer)


class PreNormFn(torch.autograd.Function):
    """The fork of a pre-norm residual block, x -> (x, LN(x)) (encoder_layer.py:79-83 etc.: `residual = x;
    x = norm(x)`).  Owning both branches lets backward produce d x = d residual + LN'(d y) in the LayerNorm
    backward kernel itself (its `add` input) instead of a separate elementwise add by autograd."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, rowmask, sole_consumer=False, fuse_fwd=False):
        x = _chk(x, "pre_norm")
        d = x.shape[-1]
        rows = x.numel() // d
        y = torch.empty_like(x)
        stats = _new(rows, 2, like=x)
        if fuse_fwd and LN_FWD_FUSE and ROWGEMM and _ln_rows_fusable(rows, d) and gamma.data_ptr() % 16 == 0 and beta.data_ptr() % 16 == 0:
            # parked: the consumer's first kernel makes y (see _PENDING_LNF)
            _PENDING_LNF.park(_LnFwdPark(x, gamma, beta, eps, rows, d, y, stats, rowmask=rowmask))
        else:
            _ln_fwd(x, gamma, beta, eps, rows, d, rowmask, ACT_NONE, y, stats)
        ctx.save_for_backward(x, gamma, beta, stats, rowmask)
        ctx.prev_drop = getattr(x, "_oe_outdrop", None) if sole_consumer else None
        ctx.ln_fuse = bool(sole_consumer and getattr(x, "_oe_lnfuse", False))
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dres, dy):
        x, gamma, beta, stats, rowmask = ctx.saved_tensors
        if dy is None:
            return dres, None, None, None, None, None, None
        d = x.shape[-1]
        rows = x.numel() // d
        dx = torch.empty_like(x)
        (dg, rg), (db, rb) = grad_sink(gamma), grad_sink(beta)
        add = None if dres is None else dres.contiguous()
        _ln_bwd(dy.contiguous(), x, gamma, beta, ACT_NONE, stats, rows, d, rowmask, add, dx, dg, db, rg is None and rb is None,
                ctx.prev_drop, fuse=ctx.ln_fuse)
        return dx, rg, rb, None, None, None, None


def pre_norm(x, gamma, beta, eps, rowmask=None, sole_consumer=False, fuse_fwd=False):
    """-> (residual, normed): use `residual` for the skip connection of the block.  sole_consumer: see layer_norm.
    fuse_fwd: the caller hands `normed` straight to an op of this module and to nothing else (EncoderLayer) - its first kernel may
    then make it (_PENDING_LNF)."""
    return PreNormFn.apply(x, gamma, beta, eps, rowmask, sole_consumer, fuse_fwd)


# Two LayerNorms back to back - an encoder layer's norm_final followed by the next layer's first pre-norm fork, or by the
# encoder's after_norm (encoder_layer.py:109-110 -> :79-80; encoder.py after the last layer) - as ONE launch each way:
# 12 forward and 12 backward launches and a round trip of the (rows, d) activation each less per step at config 2.
LN_PAIR = os.environ.get("OE_LN_PAIR", "1") == "1"


def ln_pair_ok(x):
    return LN_PAIR and x.is_cuda and x.dtype == torch.float32 and not _planes.active()


class NormPairFn(torch.autograd.Function):
    """x -> (u, y) with u = LN1(x), y = LN2(u); u is also an output when the caller needs it (the next block's residual).
    Backward: d x = LN1'(d u + LN2'(d y)) in one kernel, u recomputed from x."""

    @staticmethod
    def forward(ctx, x, g1, b1, eps1, g2, b2, eps2, want_first, sole_consumer, fuse_fwd=False):
        x = _chk(x, "layer_norm_pair")
        d = x.shape[-1]
        rows = x.numel() // d
        u = torch.empty_like(x) if want_first else None
        y = torch.empty_like(x)
        st1, st2 = _new(rows, 2, like=x), _new(rows, 2, like=x)
        if (fuse_fwd and want_first and LN_FWD_FUSE and FUSED_FFN and _ln_rows_fusable(rows, d) and
                all(t.data_ptr() % 16 == 0 for t in (g1, b1, g2, b2))):
            # parked: the next layer's first feed-forward makes u and y on its rows' way in (_PENDING_LNF, pair form)
            _PENDING_LNF.park(_LnFwdPark(x, g1, b1, eps1, rows, d, y, st1, gamma2=g2, beta2=b2, eps2=eps2, u=u, stats2=st2))
        else:
            hip.call("oe_layernorm_pair_fwd", x, g1, b1, eps1, g2, b2, eps2, rows, d, u, st1, y, st2)
        ctx.save_for_backward(x, g1, b1, st1, g2, b2, st2)
        ctx.prev_drop = getattr(x, "_oe_outdrop", None) if sole_consumer else None
        ctx.ln_fuse = bool(sole_consumer and getattr(x, "_oe_lnfuse", False))
        ctx.want_first = want_first
        if want_first:
            return u, y
        return y

    @staticmethod
    def backward(ctx, *grads):
        du, dy = grads if ctx.want_first else (None, grads[0])
        x, g1, b1, st1, g2, b2, st2 = ctx.saved_tensors
        d = x.shape[-1]
        rows = x.numel() // d
        if dy is None:
            dy = torch.zeros_like(x)
        dy = dy.contiguous()
        add = None if du is None else du.contiguous()
        dx = torch.empty_like(x)
        (dg1, rg1), (db1, rb1) = grad_sink(g1), grad_sink(b1)
        (dg2, rg2), (db2, rb2) = grad_sink(g2), grad_sink(b2)
        ws1, ws2 = _ln_ws(x, rows, d), _ln_ws(x, rows, d)
        gout, alpha, p, seed, gmask = None, 1.0, 0.0, 0, None
        arena_all = rg1 is None and rb1 is None and rg2 is None and rb2 is None
        if (ctx.ln_fuse and arena_all and ctx.prev_drop is not None and LN_BWD_FUSE and FUSE_OUT_DROP and _ln_rows_fusable(rows, d) and
                x.is_contiguous() and (add is None or add.is_contiguous())):
            # parked: the previous block's backward (the second feed-forward's oe_ffn_bwd) launches it as its prologue (_PENDING_LN)
            gout = torch.empty_like(dx)
            _PENDING_LN.park(_LnBwdPark(dy, x, g1, b1, st1, add, dx, gout, ws1, ctx.prev_drop, rows, d, dg1, db1,
                                        gamma2=g2, stats2=st2, ws2=ws2, dg2=dg2, db2=db2))
            _PREDROP[dx.data_ptr()] = (gout, ctx.prev_drop, dx, dx._version)
            return dx, rg1, rb1, None, rg2, rb2, None, None, None, None
        if ctx.prev_drop is not None and FUSE_OUT_DROP and d % 8 == 0:
            gout = torch.empty_like(dx)
            alpha, p, seed, gmask = ctx.prev_drop
        hip.call("oe_layernorm_pair_bwd_dx_drop", dy, x, g1, b1, st1, g2, st2, rows, d, add, dx, gout, alpha, p, seed, _seed_dev, gmask, ws1, ws2)
        if gout is not None:
            _PREDROP[dx.data_ptr()] = (gout, ctx.prev_drop, dx, dx._version)
        _ln_param_reduce(ws1, rows, d, dg1, db1, rg1 is None and rb1 is None)
        _ln_param_reduce(ws2, rows, d, dg2, db2, rg2 is None and rb2 is None)
        return dx, rg1, rb1, None, rg2, rb2, None, None, None, None


def layer_norm_pair(x, g1, b1, eps1, g2, b2, eps2, want_first=True, sole_consumer=False, fuse_fwd=False):
    """(LN1(x), LN2(LN1(x))) - or only the second with want_first=False.  sole_consumer: as layer_norm's.  fuse_fwd (with
    want_first): the caller hands the pair to a feed-forward as (residual, input) and to nothing else (pre_norm's fuse_fwd)."""
    return NormPairFn.apply(x, g1, b1, eps1, g2, b2, eps2, want_first, sole_consumer, fuse_fwd)


# --------------------------------------------------------------------------- #
# Linear (single GEMM with bias / activation)
# --------------------------------------------------------------------------- #
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act):
        x = _chk(x, "linear")
        x2 = x.reshape(-1, x.shape[-1])
        pre = _new(x2.shape[0], w.shape[0], like=x) if act != ACT_NONE else None
        if act in GEMM_FUSED_ACTS:
            y = gemm_nt(x2, w, b, act=act, preact_out=pre, ld_aux=w.shape[0])
        else:
            gemm_nt(x2, w, b, out=pre)
            y = torch.empty_like(pre)
            hip.call("oe_act_fwd", pre, pre.numel(), act, y)
        ctx.save_for_backward(x2, w, pre)
        ctx.act, ctx.has_bias, ctx.in_shape = act, b is not None, x.shape
        ctx.bias_ref = b
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, pre = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, w.shape[0])
        if ctx.act != ACT_NONE:
            dy2 = _act_grad(dy2, pre, ctx.act)
        dx = gemm_nn(dy2, w).view(ctx.in_shape) if ctx.needs_input_grad[0] else None
        dw, db = wgrad_bias(w, ctx.bias_ref if ctx.has_bias else None, dy2, x2)
        return dx, dw, db, None


def _act_grad(dy2, pre, act):
    """dy * act'(pre)."""
    out = torch.empty_like(dy2)
    hip.call("oe_act_grad", dy2, pre, dy2.numel(), act, out)
    return out


def linear(x, w, b=None, act=ACT_NONE):
    return LinearFn.apply(x, w, b, act)


class ActivationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        x = _chk(x, "activation")
        y = torch.empty_like(x)
        hip.call("oe_act_fwd", x, x.numel(), act, y)
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _act_grad(dy.contiguous(), x, ctx.act), None


def activation(x, act):
    return ActivationFn.apply(x, act)


class ScaleAddFn(torch.autograd.Function):
    """out = alpha * x (+ add broadcast over the batch): the x*sqrt(d) (+pe) of embedding.py:44-60,75-88 where it
    is not fused into a producing GEMM (LinearNoSubsampling)."""

    @staticmethod
    def forward(ctx, x, alpha, add):
        x = _chk(x, "scale_add input")
        out = torch.empty_like(x)
        add_b = None if add is None else _chk(add.expand_as(x), "scale_add addend")
        hip.call("oe_axpby", x, add_b, x.numel(), float(alpha), 1.0, None, out)
        ctx.alpha = float(alpha)
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        hip.call("oe_axpby", dy, None, dy.numel(), ctx.alpha, 0.0, None, dx)
        return dx, None, None


def scale_add(x, alpha, add=None):
    return ScaleAddFn.apply(x, alpha, add)


class AddFn(torch.autograd.Function):
    """x + y with both gradients passed through (encoder_layer.py:108 / decoder_layer.py:106: `x = x + adapt_x`)."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = _chk(x, "add"), _chk(y, "add")
        out = torch.empty_like(x)
        hip.call("oe_axpby", x, y, x.numel(), 1.0, 1.0, None, out)
        return out

    @staticmethod
    def backward(ctx, d):
        return d, d


def add(x, y):
    return AddFn.apply(x, y)


class LossCombineFn(torch.autograd.Function):
    """asr_model.py:150-157 + :196-198 on device scalars, one launch each way:
    att = l * (1 - r) + lr * r;  loss = wc * ctc + (1 - wc) * att  (absent terms: None)."""

    @staticmethod
    def forward(ctx, loss_att, loss_att_r, loss_ctc, ctc_weight, reverse_weight):
        f = lambda t: None if t is None else _chk(t.reshape(1), "loss")
        la, lr, lc = f(loss_att), f(loss_att_r), f(loss_ctc)
        out = _new(1, like=la)
        hip.call("oe_loss_combine", lc, la, lr, float(ctc_weight), float(reverse_weight), 1.0, out)
        ctx.cfg = (float(ctc_weight), float(reverse_weight), lr is not None, lc is not None)
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        wc, r, has_r, has_c = ctx.cfg
        g = g.contiguous().reshape(1)
        d = _new(3, like=g)
        hip.call("oe_loss_combine_bwd", g, wc, r, 1.0, d[0:1] if has_c else None, d[1:2], d[2:3] if has_r else None)
        return d[1].view(()), (d[2].view(()) if has_r else None), (d[0].view(()) if has_c else None), None, None


def combine_losses(loss_att, loss_att_r=None, loss_ctc=None, ctc_weight=0.0, reverse_weight=0.0):
    return LossCombineFn.apply(loss_att, loss_att_r, loss_ctc, ctc_weight, reverse_weight)


class CmvnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mean, istd):
        x = _chk(x, "cmvn")
        y = torch.empty_like(x)
        hip.call("oe_global_cmvn", x, mean, istd, x.numel(), x.shape[-1], y)
        return y

    @staticmethod
    def backward(ctx, dy):
        raise NotImplementedError("GlobalCMVN is applied to input features, which carry no gradient")


def global_cmvn(x, mean, istd):
    return CmvnFn.apply(x, mean, istd)


# --------------------------------------------------------------------------- #
# Position-wise feed forward (+ optional fused residual / outer dropout)
# --------------------------------------------------------------------------- #
# The fused feed-forward kernel (csrc/ffn.hip) consumes the weights pre-split to bf16 planes in MFMA-fragment order.  They
# are re-packed on every call (~3 us for the two 1 MB matrices): the optimizer moves the weights every step through a raw
# kernel, which no tensor version counter sees, so a cache could only be trusted for frozen models.
FUSED_FFN = os.environ.get("OE_FUSED_FFN", "1") == "1"
# One block of the fused kernel owns 32 rows and streams ALL of W1 and W2: it pays once there are enough rows to fill the
# chip (config 2: 7936 rows = 248 blocks, 71 us incl. the weight packing against 79 us for the two GEMMs); the decoders'
# 992 rows are 31 blocks that each still take the full ~56 us, against 41 us for their two small GEMMs.
FUSED_FFN_MIN_ROWS = int(os.environ.get("OE_FUSED_FFN_MIN_ROWS", "4096"))
# the input gradient in one launch too (oe_ffn_bwd).  None = automatic: on in precision 6 (csrc/ffn6.hip: 61 us against 92 for the
# two GEMMs at 7936 rows, profiles/r04_ffn6.md), off in precision 1 / 3 (measured slower in the step, profiles/r02_experiments.md)
FUSED_FFN_BWD = {"1": True, "0": False}.get(os.environ.get("OE_FUSED_FFN_BWD", ""), None)


def _ffn_bwd_fused() -> bool:
    return (hip.GEMM_PRECISION == 6) if FUSED_FFN_BWD is None else bool(FUSED_FFN_BWD)


def _ffn6_takes_ln(d, ff):
    """The fused feed-forward's kernel (csrc/ffn6.hip) has the LayerNorm prologues (oe_ffn_fwd's lnf, oe_ffn_bwd's ln)."""
    return hip.GEMM_PRECISION == 6 and d == 256 and ff % 256 == 0 and hip.lib().oe_ffn6_config(-1) in (0, 3)


def _ffn_fused_ok(x2, w1, w2, act, res2):
    d, ff = w1.shape[1], w1.shape[0]
    if hip.GEMM_PRECISION == 0 or x2.shape[0] < FUSED_FFN_MIN_ROWS or not hip.lib().oe_ffn_supported(d, ff, hip.GEMM_PRECISION, act):
        return False
    ok = lambda t: t is None or (t.data_ptr() % 16 == 0 and t.stride(-1) == 1)
    return (w1.is_contiguous() and w2.is_contiguous() and ok(x2) and ok(res2) and x2.stride(0) % 4 == 0 and
            (res2 is None or res2.stride(0) % 4 == 0) and w1.data_ptr() % 16 == 0 and w2.data_ptr() % 16 == 0)


# The packed weights of every feed-forward that has been seen, refreshed by ONE table-driven launch (oe_ffn_pack_weights_table) the
# first time any of them is needed after the weights may have changed (planes.weights_generation: a new forward pass, an optimizer
# step, a graph replay; plus the tensors' own version counters for writes through torch) - 48 pack launches per step at config 2
# otherwise (forward and backward orientation of 24 feed-forwards, 4.5 us each on the step's chain).

_FFN = _PackTable(9)        # rows: { W1, W2, w1p, w2p, w2tp, w1tp, d, ff, planes }; key = (W1 address, W2 address, precision)
FFN_PACK_TABLE = os.environ.get("OE_FFN_PACK_TABLE", "1") == "1"
FFN_FWD_FUSED_LAUNCHES = 0  # (tests: the fused forward / input gradient ran, on packed weights)
FFN_BWD_FUSED_LAUNCHES = 0


def _ffn_dead(key, ent):
    """A _FFN row must not be refreshed again: W1 or W2 is gone, or lives on at another address (see _row_dead)."""
    w1, w2 = ent["w1"](), ent["w2"]()
    return w1 is None or w2 is None or w1.data_ptr() != key[0] or w2.data_ptr() != key[1]


def ffn_packs_clear():
    _FFN.clear()
    row_packs_clear()


def pack_tables_sweep():
    """Neutralise the table rows of weights that have died since the last look (planes.new_pass, TrainEngine.replay: before anything
    - a captured pack launch included - can touch them: their memory may be unmapped by now, torch.cuda.empty_cache)."""
    if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
        _FFN.sweep(_ffn_dead)
        _FFN.upload()
        _ROW.sweep(_row_dead)
        _ROW.upload()


def _ffn_packed(w1, w2, d, ff, bwd=False):
    """Packed W1 / W2 (forward) or W2^T / W1^T (bwd) of one feed-forward, fresh for the weights' current values."""
    prec = hip.GEMM_PRECISION
    nbytes = hip.lib().oe_ffn_packed_bytes(d, ff, prec)
    capturing = torch.cuda.is_current_stream_capturing()
    key = (w1.data_ptr(), w2.data_ptr(), prec)
    ent = _FFN.entries.get(key) if FFN_PACK_TABLE else None
    if ent is not None and ((ent["d"], ent["ff"]) != (d, ff) or ent["w1"]() is not w1 or ent["w2"]() is not w2 or _ffn_dead(key, ent)):
        if capturing:
            ent = False                                          # (no table surgery inside a capture: a pack of this call's own)
        else:
            _FFN.drop(key)
            ent = None
    if ent is None and FFN_PACK_TABLE and not capturing and isinstance(w1, torch.nn.Parameter) and isinstance(w2, torch.nn.Parameter):
        # first sight (outside a capture: these buffers outlive every graph): persistent buffers, a table row
        bufs = [torch.empty(nbytes, dtype=torch.uint8, device=w1.device) for _ in range(4)]
        ent = dict(w1=weakref.ref(w1), w2=weakref.ref(w2), bufs=bufs, d=d, ff=ff, gen=[-1, -1], ver=[None, None])
        # (the row carries its own plane count: the table may hold feed-forwards registered under other precisions, whose
        # buffers are smaller - bench.py's extra mode-3 / mode-1 legs; a refresh in THIS precision must not overrun them)
        if not _FFN.add(key, [key[0], key[1]] + [b.data_ptr() for b in bufs] + [d, ff, {6: 3, 3: 2}.get(prec, 1)], ent, w1.device):
            ent = None
    if not ent:                                                  # unregistered (inside a capture, plain tensors): a pack of its own
        a = torch.empty(nbytes, dtype=torch.uint8, device=w1.device)
        b = torch.empty(nbytes, dtype=torch.uint8, device=w1.device)
        hip.call("oe_ffn_pack_weights_bwd" if bwd else "oe_ffn_pack_weights", w1, w2, d, ff, prec, a, b)
        return a, b
    gen, ver, kind = _planes.weights_generation(), (w1._version, w2._version), int(bwd)
    if ent["gen"][kind] != gen or ent["ver"][kind] != ver:
        if not capturing:
            _FFN.sweep(_ffn_dead)
            _FFN.upload()
        if not _FFN.dirty and len(_FFN.entries) > 1 and ent["gen"][0] != gen and ent["gen"][1] != gen:
            # nobody has refreshed anything in this generation yet: all feed-forwards, both orientations, one launch
            alive = _FFN.entries.values()
            hip.call("oe_ffn_pack_weights_table", _FFN.dev, _FFN.n, max(e["d"] for e in alive), max(e["ff"] for e in alive), prec)
            _pack_done(_FFN)
            for e in alive:
                w1e, w2e = e["w1"](), e["w2"]()
                v = (w1e._version, w2e._version) if (w1e is not None and w2e is not None) else None
                e["gen"], e["ver"] = [gen, gen], [v, v]
        else:
            _pack_wait(_FFN)                 # behind the last table launch: the event recorded below then covers every entry
            hip.call("oe_ffn_pack_weights_bwd" if bwd else "oe_ffn_pack_weights", w1, w2, d, ff, prec, ent["bufs"][2 * kind], ent["bufs"][2 * kind + 1])
            _pack_done(_FFN)
            ent["gen"][kind], ent["ver"][kind] = gen, ver
    else:
        _pack_wait(_FFN)
    return ent["bufs"][2 * kind], ent["bufs"][2 * kind + 1]


class FeedForwardFn(torch.autograd.Function):
    """y = [residual + out_scale * drop_out(] w_2(drop_in(act(w_1 x + b_1))) + b_2 [)]
    positionwise_feed_forward.py:36-43 and encoder_layer.py:81-83,104-106 / decoder_layer.py:104-106."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, p_in, residual, out_scale, p_out):
        x = _chk(x, "feed_forward", keep_pending=True)
        d = x.shape[-1]
        x2 = x.reshape(-1, d)
        M, ff = x2.shape[0], w1.shape[0]
        s_in, s_out = (next_seed() if p_in > 0 else 0), (next_seed() if p_out > 0 else 0)
        res2 = None if residual is None else _chk(residual, "residual").reshape(-1, w2.shape[0])
        lnf_p = _PENDING_LNF.take(x2)             # x may be the output of a parked LayerNorm forward (_PENDING_LNF)
        fused_now = FUSED_FFN and _ffn_fused_ok(x2, w1, w2, act, res2)
        lnf = None
        if lnf_p is not None:                     # (the pair form is for `residual = u` (EncoderLayer's pre): anything else, the plain way)
            if (fused_now and _ffn6_takes_ln(d, ff) and x2.is_contiguous() and M == lnf_p.rows and
                    (lnf_p.gamma2 is None or (res2 is not None and lnf_p.u is not None and res2.data_ptr() == lnf_p.u.data_ptr()))):
                lnf = lnf_p.prologue()
            else:
                lnf_p.resolve()
        if fused_now:
            # one kernel (csrc/ffn.hip): the (M, ff) intermediate stays in registers; pre / a are written only when a
            # backward will read them
            need = any(ctx.needs_input_grad)
            pre = _new(M, ff, like=x) if need else None
            a = _new(M, ff, like=x) if need else None
            w1p, w2p = _ffn_packed(w1, w2, d, ff)
            y = _new(M, d, like=x)
            hip.ffn_fwd(x2, w1p, b1, w2p, b2, M, d, ff, act, drop_in=p_in, seed_in=s_in, drop_out=p_out, seed_out=s_out,
                        seed_dev=_seed_dev, pre_out=pre, act_out=a, residual=res2, ldr=0 if res2 is None else res2.stride(0),
                        beta=out_scale, y=y, lnf=lnf)
            global FFN_FWD_FUSED_LAUNCHES
            FFN_FWD_FUSED_LAUNCHES += 1
            if lnf is not None:
                lnf_p.fused()
            ctx.save_for_backward(x2, w1, w2, pre, a)
            ctx.biases = (b1, b2)
            ctx.cfg = (act, p_in, s_in, out_scale, p_out, s_out, residual is not None, x.shape)
            ctx.fused = True
            # (the backward's fused kernel can take the next LayerNorm's backward as its prologue: _PENDING_LN)
            ln_fuse = LN_BWD_FUSE and FUSE_OUT_DROP and _ln_rows_fusable(M, d) and _ffn_bwd_fused() and _ffn6_takes_ln(d, ff)
            return _tag_out_drop(y.view(*x.shape[:-1], w2.shape[0]), out_scale, p_out, s_out, ln_fuse=ln_fuse)
        ctx.fused = False
        pre = _new(M, ff, like=x)
        if act in GEMM_FUSED_ACTS:
            a = gemm_nt(x2, w1, b1, act=act, preact_out=pre, ld_aux=ff, drop_p=p_in, seed=s_in, seed_dev=_seed_dev, out_planes=True)
        else:
            gemm_nt(x2, w1, b1, out=pre)
            a = torch.empty_like(pre)
            hip.call("oe_act_fwd", pre, pre.numel(), act, a)
            if p_in > 0:
                a = dropout_scale(a, 1.0, p_in, s_in)
        y = gemm_nt(a, w2, b2, drop_p=p_out, seed=s_out, seed_dev=_seed_dev, residual=res2,
                    ldr=0 if res2 is None else res2.stride(0), beta=out_scale)
        ctx.save_for_backward(x2, w1, w2, pre, a)
        ctx.biases = (b1, b2)
        ctx.cfg = (act, p_in, s_in, out_scale, p_out, s_out, residual is not None, x.shape)
        return _tag_out_drop(y.view(*x.shape[:-1], w2.shape[0]), out_scale, p_out, s_out)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, pre, a = ctx.saved_tensors
        act, p_in, s_in, out_scale, p_out, s_out, has_res, in_shape = ctx.cfg
        dy = dy.contiguous()
        dy2 = dy.view(-1, w2.shape[0])
        g2 = dy2 if (p_out == 0 and out_scale == 1.0) else _out_drop_grad(dy2, out_scale, p_out, s_out)
        b1, b2 = ctx.biases
        pend = _PENDING_LN.take(g2)               # g2 may be a parked LayerNorm backward
        if ctx.fused and _ffn_bwd_fused() and g2.stride(0) % 4 == 0:
            # both input-gradient GEMMs in one launch (csrc/ffn.hip, oe_ffn_bwd): dH is written once and never re-read here
            M, d, ff = g2.shape[0], w2.shape[0], w1.shape[0]
            w2tp, w1tp = _ffn_packed(w1, w2, d, ff, bwd=True)
            dh, dx = _new(M, ff, like=g2), _new(M, d, like=g2)
            ln = None
            if pend is not None and not pend.done:
                if _ffn6_takes_ln(d, ff) and g2.is_contiguous() and g2.data_ptr() == pend.g.data_ptr() and M == pend.rows:
                    ln = pend.prologue()
                else:
                    pend.resolve()
            # FIRST launch of this backward: it makes g2 when that is a parked LayerNorm backward (the weight gradient reads it after)
            hip.ffn_bwd(g2, w2tp, w1tp, M, d, ff, act, drop_in=p_in, seed_in=s_in, seed_dev=_seed_dev, pre=pre, dh=dh, dx=dx, ln=ln)
            global FFN_BWD_FUSED_LAUNCHES
            FFN_BWD_FUSED_LAUNCHES += 1
            if ln is not None:
                pend.fused()
            dw2, db2 = wgrad_bias(w2, b2, g2, a)
            dw1, db1 = wgrad_bias(w1, b1, dh, x2)
            return dx.view(in_shape), dw1, db1, dw2, db2, None, None, (dy if has_res else None), None, None
        if pend is not None:
            pend.resolve()
        dw2, db2 = wgrad_bias(w2, b2, g2, a)
        if act in GEMM_FUSED_ACTS:
            dh = gemm_nn(g2, w2, act=act, actgrad_in=pre, ld_aux=pre.stride(0), drop_p=p_in, seed=s_in, seed_dev=_seed_dev, out_planes=True)
        else:
            dh = gemm_nn(g2, w2)
            if p_in > 0:
                dh = dropout_scale(dh, 1.0, p_in, s_in)
            dh = _act_grad(dh, pre, act)
        dw1, db1 = wgrad_bias(w1, b1, dh, x2)
        dx = gemm_nn(dh, w1).view(in_shape)
        return dx, dw1, db1, dw2, db2, None, None, (dy if has_res else None), None, None


def feed_forward(x, w1, b1, w2, b2, act, p_in=0.0, residual=None, out_scale=1.0, p_out=0.0):
    return FeedForwardFn.apply(x, w1, b1, w2, b2, act, p_in, residual, out_scale, p_out)


# --------------------------------------------------------------------------- #
# Multi-head attention (plain and relative-position)
# --------------------------------------------------------------------------- #
def mask_bytes(mask: torch.Tensor) -> torch.Tensor:
    """A boolean / integer mask as contiguous uint8; a bool tensor is reinterpreted in place (no launch)."""
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    return (mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)).contiguous()


def _mask_u8(mask: Optional[torch.Tensor]):
    if mask is None:
        return None, (0, 0)
    m = mask_bytes(mask)
    assert m.dim() == 3, "mask must be (B, 1|T1, T2)"
    return m, (m.shape[1] * m.shape[2], 0 if m.shape[1] == 1 else m.shape[2])


# Set (by the caller that built the masks: decode paths, the LM) while every self-attention mask in flight is causal - a
# (B, L, L) mask that is zero above the diagonal: the forward kernel then skips the key blocks above it.  A hint only: the
# mask is still applied, the results are identical.
CAUSAL_SELF_ATTENTION = False


class causal_self_attention:
    def __enter__(self):
        global CAUSAL_SELF_ATTENTION
        self.old, CAUSAL_SELF_ATTENTION = CAUSAL_SELF_ATTENTION, True

    def __exit__(self, *exc):
        global CAUSAL_SELF_ATTENTION
        CAUSAL_SELF_ATTENTION = self.old
        return False


class AttentionFn(torch.autograd.Function):
    """attention.py:99-117 (MultiHeadedAttention.forward) and :166-209
    (RelPositionMultiHeadedAttention.forward) incl. linear_q/k/v/out, with an
    optional fused `residual + dropout(.)` of the caller (encoder_layer.py:89)."""

    @staticmethod
    def forward(ctx, xq, xkv, wq, bq, wk, bk, wv, bv, wo, bo, mask, pos_emb, wpos, pu, pv, H, p_attn, residual, p_out, pp_in=None):
        xq = _chk(xq, "attention query", keep_pending=True)        # (a parked LayerNorm forward: the q / k / v projection below makes it)
        self_attn = xkv is None
        B, T1, d = xq.shape
        D = d // H
        scale = 1.0 / math.sqrt(D)
        xq2 = xq.view(-1, d)
        if self_attn:
            T2 = T1
            wqkv, _ = _fused_rows((wq, wk, wv))
            bqkv, _ = _fused_rows((bq, bk, bv))
            qkv = gemm_nt(xq2, wqkv, bqkv)                       # (B*T, 3d)
            q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
            qs = ks = vs = (T1 * 3 * d, 3 * d)
            xkv2 = xq2
        else:
            xkv = _chk(xkv, "attention key/value")
            T2 = xkv.shape[1]
            xkv2 = xkv.view(-1, d)
            q = gemm_nt(xq2, wq, bq)
            wkv, _ = _fused_rows((wk, wv))
            bkv, _ = _fused_rows((bk, bv))
            kv = gemm_nt(xkv2, wkv, bkv)                         # (B*T2, 2d)
            k, v = kv[:, :d], kv[:, d:]
            qs, ks, vs = (T1 * d, d), (T2 * 2 * d, 2 * d), (T2 * 2 * d, 2 * d)
            qkv = None
        rel = pos_emb is not None
        kp = keybias = pp = None
        k_att, k_att_s = k, ks
        if rel:
            assert self_attn and pos_emb.shape[-2] == T2
            pe2 = _chk(pos_emb, "pos_emb").reshape(-1, d)
            pp = pp_in if pp_in is not None else gemm_nt(pe2, wpos)     # (T, d): linear_pos has no bias
            kp = _new(B, T2, d, like=xq)
            keybias = _new(B, H, T2, like=xq)
            hip.call("oe_relpos_prepare", k, ks[0], ks[1], pp, d, pu, pv, B, T2, H, D, scale, kp, keybias)
            k_att, k_att_s = kp, (T2 * d, d)
        m8, mstr = _mask_u8(mask)
        s_att, s_out = (next_seed() if p_attn > 0 else 0), (next_seed() if p_out > 0 else 0)
        att = _new(B, T1, d, like=xq)
        lse = _new(B, H, T1, like=xq)
        a = hip.attn_args(q, k_att, v, att, lse, B, H, T1, T2, D, scale, q_strides=qs, k_strides=k_att_s, v_strides=vs,
                          o_strides=(T1 * d, d), mask=m8, mask_strides=mstr, keybias=keybias, drop_p=p_attn, seed=s_att,
                          seed_dev=_seed_dev, causal=CAUSAL_SELF_ATTENTION and self_attn)
        hip.attention_fwd(a)
        res2 = None if residual is None else _chk(residual, "residual").view(-1, d)
        y = gemm_nt(att.view(-1, d), wo, bo, drop_p=p_out, seed=s_out, seed_dev=_seed_dev, residual=res2,
                    ldr=0 if res2 is None else d)
        ctx.save_for_backward(xq2, xkv2 if not self_attn else None, wq, wk, wv, wo, qkv, None if self_attn else q,
                              None if self_attn else kv, kp, keybias, pp, None if not rel else pe2, wpos, pu, pv, m8, att, lse)
        ctx.cfg = (self_attn, rel, B, T1, T2, d, H, D, scale, p_attn, s_att, p_out, s_out, residual is not None, mstr)
        ctx.biases = (bq, bk, bv, bo)
        ctx.pp_external = pp_in is not None
        return _tag_out_drop(y.view(B, T1, d), 1.0, p_out, s_out, ln_fuse=_ln_fuse_ok(B * T1, d, wo))

    @staticmethod
    def backward(ctx, dy):
        (xq2, xkv2, wq, wk, wv, wo, qkv, q_x, kv_x, kp, keybias, pp, pe2, wpos, pu, pv, m8, att, lse) = ctx.saved_tensors
        self_attn, rel, B, T1, T2, d, H, D, scale, p_attn, s_att, p_out, s_out, has_res, mstr = ctx.cfg
        dy = dy.contiguous()
        dy2 = dy.view(-1, d)
        g = dy2 if p_out == 0 else _out_drop_grad(dy2, 1.0, p_out, s_out)
        att2 = att.view(-1, d)
        bq, bk, bv, bo = ctx.biases
        datt = gemm_nn(g, wo)                    # FIRST: g may be a parked LayerNorm backward that this launch makes (_PENDING_LN)
        dwo, dbo = wgrad_bias(wo, bo, g, att2)
        delta = _new(B, H, T1, like=dy)
        if self_attn:
            dqkv = _new(B * T1, 3 * d, like=dy)
            q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
            dq, dk, dv = dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:]
            qs = ks = vs = (T1 * 3 * d, 3 * d)
        else:
            q, k, v = q_x, kv_x[:, :d], kv_x[:, d:]
            dq = _new(B * T1, d, like=dy)
            dkv = _new(B * T2, 2 * d, like=dy)
            dk, dv = dkv[:, :d], dkv[:, d:]
            qs, ks, vs = (T1 * d, d), (T2 * 2 * d, 2 * d), (T2 * 2 * d, 2 * d)
        k_att, k_att_s, dk_att, dkb = k, ks, dk, None
        if rel:
            dkp = _new(B, T2, d, like=dy)
            dkb = _new(B, H, T2, like=dy)
            k_att, k_att_s, dk_att = kp, (T2 * d, d), dkp
        a = hip.attn_args(q, k_att, v, att, lse, B, H, T1, T2, D, scale, q_strides=qs, k_strides=k_att_s, v_strides=vs,
                          o_strides=(T1 * d, d), mask=m8, mask_strides=mstr, keybias=keybias, drop_p=p_attn, seed=s_att,
                          seed_dev=_seed_dev, d_out=datt, dq=dq, dk=dk_att, dv=dv, dkeybias=dkb, delta=delta)
        hip.attention_bwd(a)
        dwpos = rpu = rpv = None
        if rel:
            dpp = _new(T2, d, like=dy)
            (dpu, rpu), (dpv, rpv) = grad_sink(pu), grad_sink(pv)
            hip.call("oe_relpos_backward", dkp, dkb, k, ks[0], ks[1], pp, d, pu, pv, B, T2, H, D, scale, dk, dpp, d, dpu, dpv)
            if not ctx.pp_external:
                dwpos = wgrad(wpos, dpp, pe2)

        def split_or_sink(parts_w, parts_b, dy_fused, x_in):
            """Weight/bias gradients of a fused projection: one GEMM / one column sum."""
            fw, in_place = _fused_rows(parts_w)
            dx_in = gemm_nn(dy_fused, fw)
            if in_place and _arena.grad_target(parts_w[0]) is not None:
                n = dy_fused.shape[1]
                gw = _arena.grad_target(parts_w[0])
                gw_all = torch.as_strided(gw, (n, x_in.shape[1]), (x_in.shape[1], 1))
                gb = _arena.grad_target(parts_b[0])
                gb_all = torch.as_strided(gb, (n,), (1,))
                pl = wgrad_planes(dy_fused, x_in)
                _run_wgrad(True, (dy_fused, x_in) + _pl_tensors(pl), lambda: gemm_tn(dy_fused, x_in, out=gw_all, bias_out=gb_all, planes=pl),
                           desc=dict(dy=dy_fused, x=x_in, out=gw_all, alpha=1.0, alpha_dev=None, bias_out=gb_all))
                return dx_in, [None] * len(parts_w), [None] * len(parts_b)
            dwf, dbf = gemm_tn(dy_fused, x_in), colsum(dy_fused)
            ws, bs, o = [], [], 0
            for pw, pb in zip(parts_w, parts_b):
                r = pw.shape[0]
                tw, tb = _arena.grad_target(pw), _arena.grad_target(pb)
                if tw is not None:
                    tw.add_(dwf[o:o + r]); tb.add_(dbf[o:o + r]); ws.append(None); bs.append(None)
                else:
                    ws.append(dwf[o:o + r]); bs.append(dbf[o:o + r])
                o += r
            return dx_in, ws, bs

        if self_attn:
            dx, (dwq, dwk, dwv), (dbq, dbk, dbv) = split_or_sink((wq, wk, wv), (bq, bk, bv), dqkv, xq2)
            dx = dx.view(B, T1, d)
            dxkv = None
        else:
            dx = gemm_nn(dq, wq).view(B, T1, d)
            dwq, dbq = wgrad_bias(wq, bq, dq, xq2)
            dxkv, (dwk, dwv), (dbk, dbv) = split_or_sink((wk, wv), (bk, bv), dkv, xkv2)
            dxkv = dxkv.view(B, T2, d)
        return (dx, dxkv, dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo, None, None, dwpos, rpu, rpv, None, None,
                (dy if has_res else None), None, (dpp if (rel and ctx.pp_external) else None))


def attention(xq, xkv, wq, bq, wk, bk, wv, bv, wo, bo, mask, H, p_attn=0.0, pos_emb=None, wpos=None, pu=None, pv=None,
              residual=None, p_out=0.0, pp=None):
    return AttentionFn.apply(xq, xkv, wq, bq, wk, bk, wv, bv, wo, bo, mask, pos_emb, wpos, pu, pv, H, p_attn, residual, p_out, pp)


class ScoresAttentionFn(torch.autograd.Function):
    """attention.py:65-97 up to (not including) linear_out, on MATERIALISED scores: masked softmax -> 0-fill -> dropout ->
    attn @ value -> heads merged.  Module-API surface only (MultiHeadedAttention.forward_attention); forward() uses
    AttentionFn, which never builds the (B,H,T1,T2) tensor.  value (B,H,T2,dk) in any strides with a contiguous last
    dim (forward_qkv returns transposed views); returns (B,T1,H*dk)."""

    @staticmethod
    def forward(ctx, value, scores, mask, p):
        scores = _chk(scores, "scores")
        if not value.is_cuda or value.dtype != torch.float32:
            raise TypeError("value: openeat_amd ops need float32 CUDA tensors; there is no CPU fallback")
        if value.stride(-1) != 1:
            value = value.contiguous()
        B, H, T1, T2 = scores.shape
        dk = value.shape[-1]
        m8, mstr = _mask_u8(mask)
        seed = next_seed() if p > 0 else 0
        y = torch.empty_like(scores)
        att = torch.empty_like(scores) if p > 0 else y
        hip.call("oe_masked_softmax_fwd", scores, m8, mstr[0], mstr[1], B, H, T1, T2, float(p), seed, _seed_dev, y, att)
        out = _new(B, T1, H, dk, like=scores)
        for b in range(B):
            for h in range(H):
                v = value[b, h]
                hip.gemm(att[b, h], v, out[b, :, h], T1, dk, T2, lda=T2, ldb=v.stride(0), ldc=H * dk, b_kmajor=True)
        ctx.save_for_backward(value, y, att)
        ctx.cfg = (p, seed)
        return out.view(B, T1, H * dk)

    @staticmethod
    def backward(ctx, dout):
        value, y, att = ctx.saved_tensors
        p, seed = ctx.cfg
        B, H, T1, T2 = y.shape
        dk = value.shape[-1]
        dout = dout.contiguous().view(B, T1, H, dk)
        datt = torch.empty_like(y)
        dv = torch.zeros(B, H, T2, dk, device=y.device, dtype=torch.float32)
        for b in range(B):
            for h in range(H):
                g, v = dout[b, :, h], value[b, h]
                hip.gemm(g, v, datt[b, h], T1, T2, dk, lda=H * dk, ldb=v.stride(0), ldc=T2)                       # dO @ V^T
                hip.gemm(att[b, h], g, dv[b, h], T2, dk, T1, lda=T2, ldb=H * dk, ldc=dk, a_kmajor=True, b_kmajor=True,
                         atomic_out=True)                                                                         # P^T @ dO
        ds = torch.empty_like(y)
        hip.call("oe_masked_softmax_bwd", y, datt, B * H * T1, T2, float(p), seed, _seed_dev, ds)
        return dv, ds, None, None


def scores_attention(value, scores, mask, p=0.0):
    return ScoresAttentionFn.apply(value, scores, mask, p)


# linear_pos(pos_emb) (attention.py:185) depends on the positional table and one weight only: with POS_PROJ_AHEAD the
# encoder computes it for every layer on the side stream when it starts, as an autograd node of its own - so the
# projection AND its weight gradient (which autograd runs on the same stream) leave the layers' critical chain.
# Off for eager multi-rank steps: there the backward hooks hand finished slices of the gradient arena to the collective,
# and this node's weight gradient would run after its layer's slice had gone.
POS_PROJ_AHEAD = False


class PosProjFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos_emb, wpos):
        pe2 = _chk(pos_emb, "pos_emb").reshape(-1, wpos.shape[1])
        ctx.save_for_backward(pe2, wpos)
        return gemm_nt(pe2, wpos)

    @staticmethod
    def backward(ctx, dpp):
        pe2, wpos = ctx.saved_tensors
        return None, wgrad(wpos, dpp.contiguous(), pe2)


def pos_proj(pos_emb, wpos):
    return PosProjFn.apply(pos_emb, wpos)


# --------------------------------------------------------------------------- #
# Conformer convolution module
# --------------------------------------------------------------------------- #
DWCONV_LN_FUSED = os.environ.get("OE_DWCONV_LN", "1") == "1"


class ConvModuleFn(torch.autograd.Function):
    """convolution.py:72-120: mask -> pw1 -> GLU -> depthwise -> LayerNorm -> act -> pw2 -> mask
    (+ optional fused `residual + dropout(.)`, encoder_layer.py:95)."""

    @staticmethod
    def forward(ctx, x, rowmask, w1, b1, wd, bd, g, b, w2, b2, K, causal, act, residual, p_out, input_masked):
        x = _chk(x, "conv_module", keep_pending=not (rowmask is not None and not input_masked))    # (pointwise_conv1 below makes a parked LayerNorm)
        B, T, d = x.shape
        x2 = x.view(-1, d)
        xm = x2 if (rowmask is None or input_masked) else dropout_scale(x2, 1.0, 0.0, 0, rowmask)
        w1m, w2m = w1.view(2 * d, d), w2.view(d, d)
        a = gemm_nt(xm, w1m, b1)                                  # (B*T, 2d)
        yc = _new(B * T, d, like=x)
        gpad = None
        if causal:   # the reference pads before pointwise_conv1: padded frames hold GLU(bias)
            gpad = _new(d, like=x)
            hip.call("oe_glu_fwd", b1, 1, d, gpad)
        z = torch.empty_like(yc)
        stats = _new(B * T, 2, like=x)
        if DWCONV_LN_FUSED and not _planes.active():
            # the depthwise convolution normalises its own rows: one launch and one pass over (B*T, d) less per layer
            hip.call("oe_dwconv_glu_ln_fwd", a, wd, bd, gpad, B, T, d, K, int(causal), yc, g, b, 1e-5, act, z, stats)
        else:
            hip.call("oe_dwconv_glu_fwd", a, wd, bd, gpad, B, T, d, K, int(causal), yc)
            _ln_fwd(yc, g, b, 1e-5, B * T, d, None, act, z, stats)
        s_out = next_seed() if p_out > 0 else 0
        res2 = None if residual is None else _chk(residual, "residual").view(-1, d)
        y = gemm_nt(z, w2m, b2, drop_p=p_out, seed=s_out, seed_dev=_seed_dev, rowmask=rowmask, residual=res2,
                    ldr=0 if res2 is None else d)
        ctx.save_for_backward(xm, rowmask, w1, wd, g, b, w2, a, yc, stats, z, gpad)
        ctx.biases = (b1, bd, b2)
        ctx.cfg = (B, T, d, K, causal, act, p_out, s_out, residual is not None)
        return _tag_out_drop(y.view(B, T, d), 1.0, p_out, s_out, rowmask, ln_fuse=_ln_fuse_ok(B * T, d, w2m))

    @staticmethod
    def backward(ctx, dy):
        xm, rowmask, w1, wd, g, b, w2, a, yc, stats, z, gpad = ctx.saved_tensors
        b1, bd, b2 = ctx.biases
        B, T, d, K, causal, act, p_out, s_out, has_res = ctx.cfg
        dy = dy.contiguous()
        dy2 = dy.view(-1, d)
        w1m, w2m = w1.view(2 * d, d), w2.view(d, d)
        gq = dy2 if (p_out == 0 and rowmask is None) else _out_drop_grad(dy2, 1.0, p_out, s_out, rowmask)
        dyc = torch.empty_like(yc)
        (dg, rg), (dbeta, rbeta) = grad_sink(g), grad_sink(b)
        to_arena = rg is None and rbeta is None
        # the norm + activation behind the depthwise convolution: its backward as the EPILOGUE of pointwise_conv2's input gradient
        # (oe_rowgemm6's lne arguments: the block owns whole rows), when that launch is the 256 <- 256 row-block kernel
        epi_ln = None
        if LN_EPI_FUSE and ROWGEMM and _ln_rows_fusable(B * T, d) and act in GEMM_FUSED_ACTS and to_arena:
            epi_ln = dict(x=yc, stats=stats, gamma=g, beta=b, act=act, dx=dyc, ws=_ln_ws(yc, B * T, d), done=False)
        dz = gemm_nn(gq, w2m, ln_epi=epi_ln)     # FIRST: gq may be a parked LayerNorm backward that this launch makes (_PENDING_LN)
        dw2, db2 = wgrad_bias(w2, b2, gq, z)
        if epi_ln is not None and epi_ln["done"]:
            global LN_EPI_FUSED_LAUNCHES
            LN_EPI_FUSED_LAUNCHES += 1
            _ln_param_reduce(epi_ln["ws"], B * T, d, dg, dbeta, to_arena)
        else:
            _ln_bwd(dz, yc, g, b, act, stats, B * T, d, None, None, dyc, dg, dbeta, to_arena)
        da = torch.empty_like(a)
        (dwd, rwd), (dbd, rbd) = grad_sink(wd), grad_sink(bd)
        dgpad = torch.zeros(d, device=dy.device) if causal else None
        ws = _new(hip.lib().oe_dwconv_glu_bwd_workspace_floats(B, T, d, K), like=dy)
        hip.call("oe_dwconv_glu_bwd", a, dyc, wd, gpad, B, T, d, K, int(causal), da, dwd, dbd, dgpad, ws)
        (db1, rb1) = grad_sink(b1)
        tw1 = _arena.grad_target(w1)
        ow1 = tw1.view(2 * d, d) if tw1 is not None else _new(2 * d, d, like=dy, zero=True)
        pl = wgrad_planes(da, xm)
        _run_wgrad(tw1 is not None and rb1 is None and not causal, (da, xm) + _pl_tensors(pl), lambda: gemm_tn(da, xm, out=ow1, bias_out=db1, planes=pl),
                   desc=dict(dy=da, x=xm, out=ow1, alpha=1.0, alpha_dev=None, bias_out=db1))
        dw1 = None if tw1 is not None else ow1.view(w1.shape)
        if causal:
            db1_pad = torch.empty_like(db1)
            hip.call("oe_glu_bwd", b1, dgpad, 1, d, db1_pad)
            hip.call("oe_axpby", db1_pad, db1, 2 * d, 1.0, 1.0, None, db1)
        dx = gemm_nn(da, w1m, rowmask=rowmask).view(B, T, d)
        return dx, None, dw1, rb1, rwd, rbd, rg, rbeta, dw2, db2, None, None, None, (dy if has_res else None), None, None


def conv_module(x, rowmask, w1, b1, wd, bd, g, b, w2, b2, K, causal, act, residual=None, p_out=0.0, input_masked=False):
    return ConvModuleFn.apply(x, rowmask, w1, b1, wd, bd, g, b, w2, b2, K, causal, act, residual, p_out, input_masked)


# --------------------------------------------------------------------------- #
# Conv2d subsampling (1/4) + output Linear + positional scaling
# --------------------------------------------------------------------------- #
CONV_DGRAD_IMPLICIT = os.environ.get("OE_CONV_DGRAD", "implicit") != "col2im"
# pre-split conv GEMMs walk the reduction channel-chunk major (oe_gemm_args.conv_korder): the taps of one 32-channel chunk back to
# back, so the overlapping windows of neighbouring output positions hit L2.  Only for problems the pre-split kernel surely takes.
CONV_KORDER = os.environ.get("OE_CONV_KORDER", "1") == "1"
CONV_KORDER_MIN_ROWS = 32768


def _korder_cols(w2d, taps, C):
    """(rows, taps * C) with columns (tap, c) -> columns (c // 32, tap, c % 32)."""
    r = w2d.shape[0]
    return w2d.view(r, taps, C // 32, 32).permute(0, 2, 1, 3).contiguous().view(r, taps * C)
# the conv weight gradient on pre-split operands too (dy leaves the Linear's input-gradient GEMM with planes): 256 x 256 tiles
# with the kernel's own split of the 150784-deep reduction, 1454 -> 817 us at config 2 (same-box A/B, step 21.9 -> 21.55 ms)
CONV_WGRAD_PLANES = os.environ.get("OE_CONV_WGRAD_PLANES", "1") == "1"
# the conv1 activation as bf16 planes only, its ReLU mask read from plane 0 (ConvSubsamplingFn.forward)
CONV1_PLANES_ONLY = os.environ.get("OE_CONV1_PLANES_ONLY", "1") == "1"
# the zero-padded dy of the stride-2 input gradient written as bf16 planes directly (_conv_dgrad_k3s2)
CONV_PAD_PLANES = os.environ.get("OE_CONV_PAD_PLANES", "1") == "1"


def _conv_dgrad_k3s2(dy, wk, yin, B, Ti, Fi, To, Fo, C, yin_planes=None):
    """Input gradient of Conv2d(C, C, 3, stride 2) (+ the ReLU mask of its input) without a column buffer.
    dx[b, t1, f1, ci] = sum over the taps (kh, kw) with t1 - kh and f1 - kw even of dy[b, (t1-kh)/2, (f1-kw)/2, :] . W[:, ci, kh, kw]:
    per parity class (t1 % 2, f1 % 2) that is a stride-1 convolution of dy with a 2x2 / 1x2 / 2x1 / 1x1 kernel, i.e. an
    implicit GEMM whose A rows are gathered from dy padded with one zero position on every side (so every tap is in
    bounds and the gather needs no predicate) and whose epilogue scatters the rows to dx[:, t1 % 2 :: 2, f1 % 2 :: 2]
    and applies the mask.  The same 2*M*N*K flops as the column-buffer form, 1.4 GB less written and 2.7 GB less gathered
    at config 2."""
    # every class on pre-split operands in channel-chunk order (the launch fails rather than fall back): the padded dy is made
    # as bf16 planes directly - no padded fp32 tensor, no split pass over it
    ni_min, nj_min = Ti // 2, Fi // 2
    direct = bool(_planes.available() and CONV_PAD_PLANES and CONV_KORDER and C % 32 == 0 and B * ni_min * nj_min >= CONV_KORDER_MIN_ROWS)
    dyp_pl = None
    if direct:
        dyp = None
        dyp_pl = _planes.alloc(B * (To + 2) * (Fo + 2), C, dy.device)
        hip.call("oe_pad1_nhwc_planes", dy, B, To, Fo, C, None, dyp_pl.t, dyp_pl.stride)
    else:
        dyp = _new(B, To + 2, Fo + 2, C, like=dy)
        hip.call("oe_pad1_nhwc", dy, B, To, Fo, C, dyp)
    wcls = _new(9 * C * C, like=dy)                    # the four classes' B operands [ci][(window row, window col, co)], one launch
    hip.call("oe_conv_dgrad_k3s2_weights", wk, C, wcls)
    # yin_planes: the stage's input exists as bf16 planes only - the ReLU mask is read from plane 0 (same sign, half the bytes)
    dyin = torch.empty_like(yin) if yin_planes is None else _new(B, Ti, Fi, C, like=dy)
    flat_in, flat_out = (None if dyp is None else dyp.view(-1)), dyin.view(-1)
    flat_y = yin.reshape(-1) if yin_planes is None else yin_planes.t[0].reshape(-1)
    if dyp_pl is None:
        dyp_pl = _planes.of(dyp.view(-1, C)) if _planes.available() else None   # pre-split mode: one pass over the padded dy
    w_off = 0
    for pt in (0, 1):
        KH = 2 if pt == 0 else 1                       # window row 0 is dy row i - 1 (tap 2), row 1 is dy row i (tap 0); odd t1: tap 1
        ni = (Ti + 1 - pt) // 2
        for pf in (0, 1):
            KW = 2 if pf == 0 else 1
            nj = (Fi + 1 - pf) // 2
            wsel = wcls[w_off:w_off + KH * KW * C * C].view(C, KH * KW * C)
            w_off += KH * KW * C * C
            a_off = (pt * (Fo + 2) + pf) * C           # odd classes start one padded row / column further
            o_off = (pt * Fi + pf) * C
            ap = bp = None
            korder = 0
            if dyp_pl is not None:
                korder = int(CONV_KORDER and C % 32 == 0 and B * ni * nj >= CONV_KORDER_MIN_ROWS)
                bp = _planes.of(_korder_cols(wsel, KH * KW, C) if korder else wsel, force=True)
                if bp is not None:             # the class's window into the padded dy: the same planes, a_off elements in
                    ap = _planes.Planes(dyp_pl.t, dyp_pl.ptr + 2 * a_off, dyp_pl.stride, C, dyp_pl.rows, C)
                else:
                    korder = 0
            assert flat_in is not None or (korder and ap is not None)
            hip.gemm(None if flat_in is None else flat_in[a_off:], wsel, flat_out[o_off:], B * ni * nj, C, KH * KW * C, lda=0, ldb=KH * KW * C, ldc=C,
                     act=ACT_RELU, actgrad_in=flat_y[o_off:], ld_aux=C, conv=(To + 2, Fo + 2, ni, nj, C, KW, 1), conv_gather=hip.GATHER_A,
                     conv_kh=KH, scatter=(Ti, Fi, ni, nj, 2), a_planes=ap, b_planes=bp, conv_korder=korder, actgrad_bf16=yin_planes is not None)
    return dyin


class ConvSubsamplingFn(torch.autograd.Function):
    """subsampling.py:110-116 (Conv2dSubsampling4) / :176-182 (6) / :248-253 (8) + embedding.py:44-60/75-88:
    Conv2d(1,C,3,2)+ReLU -> n x [Conv2d(C,C,k,s)+ReLU] -> channel-major flatten -> Linear -> x*sqrt(d) (+pe);
    `geoms` = ((k, s), ...) of the n C->C stages ((3,2) for 1/4, (5,3) for 1/6, (3,2),(3,2) for 1/8).
    Activations are kept NHWC so every C->C conv is an implicit GEMM (im2col gather in the operand load) and the
    flatten before the Linear is free; the checkpoint's OIHW / channel-major weights are re-laid-out on the fly (tiny).
    Arguments after the fixed ones: (w_k, b_k) of the n C->C conv stages, in forward order."""

    @staticmethod
    def forward(ctx, x, w1, b1, wl, bl, pe, xscale, geoms, *stage_params):
        x = _chk(x, "subsampling input")
        B, T, Fd = x.shape
        C = w1.shape[0]
        d = wl.shape[0]
        n = len(stage_params) // 2
        assert len(geoms) == n
        dims = [((T - 3) // 2 + 1, (Fd - 3) // 2 + 1)]
        T1, F1 = dims[0]
        # The conv1 activation as bf16 planes ONLY (no fp32 copy: 636 MB less written here and 318 MB less read by the input
        # gradient's ReLU mask at config 2) when every reader is sure to take the pre-split kernel: the first C -> C stage is the
        # 3x3 stride-2 one in channel-chunk order forward and in all four parity classes backward (oe_gemm_f32 fails loudly
        # otherwise), and its weight gradient runs on planes too.
        planes_only = False
        if _planes.available() and n > 0 and CONV1_PLANES_ONLY and geoms[0] == (3, 2) and CONV_DGRAD_IMPLICIT and CONV_WGRAD_PLANES \
                and CONV_KORDER and C % 32 == 0 and C % 128 == 0 and T1 >= 3 and F1 >= 3:
            To0, Fo0 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
            # (the weight gradient reduces over the B To0 Fo0 output positions and has no other kernel to fall back to: any count
            # goes since planes buffers carry zero pad rows to the next multiple of 16, oe_gemm_args.planes_k_padded)
            planes_only = (B * To0 * Fo0 >= CONV_KORDER_MIN_ROWS and B * (T1 // 2) * (F1 // 2) >= CONV_KORDER_MIN_ROWS)
        if planes_only:
            y = None
            y_pl = _planes.alloc(B * T1 * F1, C, x.device)
            hip.call("oe_conv1_fwd_pl", x, w1, b1, B, T, Fd, C, None, y_pl.t, y_pl.stride)
            acts = [y_pl.t]
        else:
            y = _new(B, T1, F1, C, like=x)
            y_pl = _planes.new_output(y.view(-1, C)) if (_planes.available() and n > 0) else None     # conv2 reads it pre-split
            if y_pl is not None:
                hip.call("oe_conv1_fwd_pl", x, w1, b1, B, T, Fd, C, y, y_pl.t, y_pl.stride)
            else:
                hip.call("oe_conv1_fwd", x, w1, b1, B, T, Fd, C, y)
            acts = [y]
        wgs = []
        for k in range(n):
            wk, bk = stage_params[2 * k], stage_params[2 * k + 1]
            Ti, Fi = dims[-1]
            ks, st = geoms[k]
            To, Fo = (Ti - ks) // st + 1, (Fi - ks) // st + 1
            assert Ti >= ks and Fi >= ks and To > 0 and Fo > 0, "input too short for the subsampling stack"
            kk = ks * ks
            wg = _new(C, kk * C, like=x)                            # [co][kh][kw][ci]
            hip.call("oe_swap_last2", wk, C, C, kk, wg, 0)
            yo = _new(B * To * Fo, C, like=x)
            ap = bp = cp = None
            korder = 0
            if _planes.available():            # pre-split mode: the NHWC activation and the re-laid weights as bf16 planes
                ap = y_pl if (k == 0 and planes_only) else _planes.of(acts[-1].view(-1, C))
                korder = int(ap is not None and CONV_KORDER and C % 32 == 0 and B * To * Fo >= CONV_KORDER_MIN_ROWS)
                bp = _planes.of(_korder_cols(wg, kk, C) if korder else wg, force=True) if ap is not None else None
                if bp is None:
                    ap, korder = None, 0
                cp = _planes.new_output(yo) if (k + 1 < n or _planes.split_activations()) else None    # a next conv stage reads it as an operand
            assert not (k == 0 and planes_only) or (korder and bp is not None)
            hip.gemm(None if (k == 0 and planes_only) else acts[-1], wg, yo, B * To * Fo, C, kk * C, lda=0, ldb=kk * C, ldc=C, bias=bk, act=ACT_RELU,
                     conv=(Ti, Fi, To, Fo, C, ks, st), conv_gather=hip.GATHER_A, a_planes=ap, b_planes=bp, c_planes=cp, conv_korder=korder)
            dims.append((To, Fo))
            acts.append(yo.view(B, To, Fo, C))
            wgs.append(wg)
        TL, FL = dims[-1]
        assert wl.shape[1] == C * FL, "Linear input size does not match the conv output"
        wlg = _new(d, FL * C, like=x)                               # columns reordered to (f, c)
        hip.call("oe_swap_last2", wl, d, C, FL, wlg, 0)
        ylv = acts[-1].view(B * TL, FL * C)
        pe2 = None if pe is None else _chk(pe, "pe").reshape(-1, d)[:TL]
        out = gemm_nt(ylv, wlg, bl, beta=xscale, residual=pe2, ldr=0 if pe2 is None else d, res_row_mod=0 if pe2 is None else TL)
        ctx.save_for_backward(x, wlg, *acts, *wgs)
        ctx.params = (w1, b1, wl, bl, stage_params)
        ctx.cfg = (B, T, Fd, C, d, xscale, n, dims, geoms)
        ctx.planes_only = planes_only
        return out.view(B, TL, d)

    @staticmethod
    def backward(ctx, dout):
        B, T, Fd, C, d, xscale, n, dims, geoms = ctx.cfg
        x, wlg = ctx.saved_tensors[0], ctx.saved_tensors[1]
        acts = ctx.saved_tensors[2:2 + n + 1]
        wgs = ctx.saved_tensors[2 + n + 1:]
        w1, b1, wl, bl, stage_params = ctx.params
        TL, FL = dims[-1]
        do2 = dout.contiguous().view(B * TL, d)
        ylv = acts[-1].view(B * TL, FL * C)
        (dbl_buf, dbl) = grad_sink(bl)
        dwlg = gemm_tn(do2, ylv, alpha=xscale, bias_out=dbl_buf)
        dwl = _sink_swapped(wl, dwlg, d, FL, C)
        # gradient w.r.t. the last conv's pre-activation: the Linear's dgrad with the ReLU mask fused
        dy = gemm_nn(do2, wlg, alpha=xscale, act=ACT_RELU, actgrad_in=ylv, ld_aux=FL * C,
                     out_planes="always" if CONV_WGRAD_PLANES else True).view(B * TL * FL, C)
        fused = hip.GEMM_PRECISION != 0
        stage_grads = [None] * (2 * n)
        for k in range(n - 1, -1, -1):
            wk, bk = stage_params[2 * k], stage_params[2 * k + 1]
            (Ti, Fi), (To, Fo) = dims[k], dims[k + 1]
            ks, st = geoms[k]
            kk = ks * ks
            Mo = B * To * Fo
            conv = (Ti, Fi, To, Fo, C, ks, st)
            yin = acts[k]
            dwg = _new(C, kk * C, like=do2, zero=True)
            (dbk_buf, dbk) = grad_sink(bk)
            yin_pl = None
            if k == 0 and ctx.planes_only:          # acts[0] is the (3, rows, C) bf16 planes tensor: there is no fp32 copy
                yin_pl = _planes.Planes(yin, yin.data_ptr(), yin.shape[1] * C, C, yin.shape[1], C, kpad=True)     # (planes.alloc's buffer)
                ap, bp = _planes.of(dy, make=True, force=True), yin_pl
                assert ap is not None, "the conv stage's output gradient must be dense, 16-byte aligned fp32"
                yin = None
            else:
                ap, bp = wgrad_planes(dy, yin.view(-1, C), always=CONV_WGRAD_PLANES)
            hip.gemm(dy, yin, dwg, C, kk * C, Mo, lda=C, ldb=0, ldc=kk * C, a_kmajor=True, b_kmajor=True,
                     split_k=_split_k(C, kk * C, Mo), atomic_out=True, conv=conv, conv_gather=hip.GATHER_B,
                     a_colsum=dbk_buf if fused else None, a_planes=ap, b_planes=bp)
            if not fused:
                colsum(dy, out=dbk_buf)
            stage_grads[2 * k], stage_grads[2 * k + 1] = _sink_swapped(wk, dwg, C, kk, C), dbk
            if yin_pl is not None:
                dyin = _conv_dgrad_k3s2(dy, wk, None, B, Ti, Fi, To, Fo, C, yin_planes=yin_pl)
            elif (ks, st) == (3, 2) and CONV_DGRAD_IMPLICIT:
                dyin = _conv_dgrad_k3s2(dy, wk, yin, B, Ti, Fi, To, Fo, C)
            else:
                dcol = gemm_nn(dy, wgs[k])                           # (Mo, k*k*C)
                dyin = torch.empty_like(yin)
                hip.call("oe_col2im_relu_ks", dcol, yin, B, Ti, Fi, C, ks, st, dyin)   # col2im + the ReLU mask of this stage's input
                del dcol
            dy = dyin.view(B * Ti * Fi, C)
        (dw1, rw1), (db1, rb1) = grad_sink(w1), grad_sink(b1)
        hip.call("oe_conv1_wgrad", x, dy.view(B, dims[0][0], dims[0][1], C), B, T, Fd, C, dw1, db1)
        return (None, rw1, rb1, dwl, dbl, None, None, None) + tuple(stage_grads)


def subsampling4(x, w1, b1, w2, b2, wl, bl, pe, xscale):
    return ConvSubsamplingFn.apply(x, w1, b1, wl, bl, pe, xscale, ((3, 2),), w2, b2)


def subsampling6(x, w1, b1, w2, b2, wl, bl, pe, xscale):
    return ConvSubsamplingFn.apply(x, w1, b1, wl, bl, pe, xscale, ((5, 3),), w2, b2)


def subsampling8(x, w1, b1, w2, b2, w3, b3, wl, bl, pe, xscale):
    return ConvSubsamplingFn.apply(x, w1, b1, wl, bl, pe, xscale, ((3, 2), (3, 2)), w2, b2, w3, b3)


# --------------------------------------------------------------------------- #
# heads
# --------------------------------------------------------------------------- #
def _vpad(V: int) -> int:
    return (V + 3) // 4 * 4


class CTCHeadFn(torch.autograd.Function):
    """ctc.py:38-45: ctc_lo -> log_softmax -> CTCLoss(sum, zero_infinity) / B, fused with its
    gradient; the logits buffer is overwritten by d loss/d logits (never read again)."""

    @staticmethod
    def forward(ctx, hs, w, b, hlens, ys, ylens, length_normalized=False):
        hs = _chk(hs, "ctc input")
        B, T, d = hs.shape
        V = w.shape[0]
        Vp = _vpad(V)
        hs2 = hs.view(-1, d)
        logits = _new(B * T, Vp, like=hs)
        hip.gemm(hs2, w, logits, B * T, V, d, lda=d, ldb=d, ldc=Vp, bias=b)
        if Vp != V:
            logits[:, V:].zero_()
        Lmax = max(int(ys.shape[1]), 1)
        ys32 = ys.to(torch.int32).contiguous()
        if ys32.shape[1] == 0:
            ys32 = torch.zeros(B, 1, dtype=torch.int32, device=hs.device)
        hl32, yl32 = hlens.to(torch.int32).contiguous(), ylens.to(torch.int32).contiguous()
        ws = _new(hip.lib().oe_ctc_workspace_floats(B, T, Lmax), like=hs)
        nll = _new(B, like=hs)
        tot = _new(1, like=hs)
        # reduction 'sum' then / B (ctc.py:43-44); 'mean' = mean_b(nll_b / max(len_b, 1)), then / B as well
        uw = (1.0 / yl32.clamp(min=1).to(torch.float32)) if length_normalized else None
        denom = float(B * B) if length_normalized else float(B)
        hip.call("oe_ctc_loss_fused", logits, Vp, B, T, V, hl32, ys32, Lmax, yl32, 1.0 / denom, uw, nll, tot, logits, ws)
        ctx.save_for_backward(hs2, w, logits)
        ctx.shape = (B, T, d, V)
        ctx.bias_ref = b
        return tot[0] / denom

    @staticmethod
    def backward(ctx, g):
        stamp("bwd: ctc head backward starts")
        hs2, w, dlogits = ctx.saved_tensors
        B, T, d, V = ctx.shape
        g = g.contiguous().view(1)
        dl = dlogits[:, :V]
        dhs = gemm_nn_deep(dl, w, alpha_dev=g).view(B, T, d)
        dw, db = wgrad_bias(w, ctx.bias_ref, dl, hs2, alpha_dev=g)
        return dhs, dw, db, None, None, None, None


def ctc_head(hs, w, b, hlens, ys, ylens, length_normalized=False):
    return CTCHeadFn.apply(hs, w, b, hlens, ys, ylens, length_normalized)


class LSMHeadFn(torch.autograd.Function):
    """decoder.py:192 (output_layer) + label_smoothing_loss.py:58-91 + common.py:135-157, fused.
    Returns (loss, n_correct, n_valid)."""

    @staticmethod
    def forward(ctx, x, w, b, target, smoothing, normalize_length, ignore_id):
        x = _chk(x, "decoder output")
        B = x.shape[0]
        d = x.shape[-1]
        V = w.shape[0]
        Vp = _vpad(V)
        x2 = x.reshape(-1, d)
        rows = x2.shape[0]
        logits = _new(rows, Vp, like=x)
        hip.gemm(x2, w, logits, rows, V, d, lda=d, ldb=d, ldc=Vp, bias=b)
        tgt = target.reshape(-1).to(torch.int64).contiguous()
        ws = torch.empty(hip.lib().oe_lsm_workspace_bytes(rows), dtype=torch.uint8, device=x.device)
        out3 = _new(3, like=x)
        hip.call("oe_lsm_loss_fused", logits, Vp, rows, V, tgt, ignore_id, smoothing, int(normalize_length), float(B), 1.0,
                 1, out3, ws)
        ctx.save_for_backward(x2, w, logits)
        ctx.shape = (x.shape, V)
        ctx.bias_ref = b
        ctx.mark_non_differentiable(out3[1], out3[2])
        return out3[0], out3[1], out3[2]

    @staticmethod
    def backward(ctx, g, _g1, _g2):
        stamp("bwd: a decoder's backward starts")
        x2, w, dlogits = ctx.saved_tensors
        shape, V = ctx.shape
        g = g.contiguous().view(1)
        dl = dlogits[:, :V]
        dx = gemm_nn_deep(dl, w, alpha_dev=g).view(shape)
        dw, db = wgrad_bias(w, ctx.bias_ref, dl, x2, alpha_dev=g)
        return dx, dw, db, None, None, None, None


def lsm_head(x, w, b, target, smoothing, normalize_length=False, ignore_id=-1):
    return LSMHeadFn.apply(x, w, b, target, smoothing, normalize_length, ignore_id)


class LSMLossFn(torch.autograd.Function):
    """label_smoothing_loss.py:58-91 on materialised logits (module API)."""

    @staticmethod
    def forward(ctx, x, target, smoothing, normalize_length, ignore_id):
        x = _chk(x, "logits")
        B, V = x.shape[0], x.shape[-1]
        Vp = _vpad(V)
        rows = x.numel() // V
        buf = _new(rows, Vp, like=x, zero=(Vp != V))
        buf[:, :V].copy_(x.reshape(rows, V))
        tgt = target.reshape(-1).to(torch.int64).contiguous()
        ws = torch.empty(hip.lib().oe_lsm_workspace_bytes(rows), dtype=torch.uint8, device=x.device)
        out3 = _new(3, like=x)
        hip.call("oe_lsm_loss_fused", buf, Vp, rows, V, tgt, ignore_id, smoothing, int(normalize_length), float(B), 1.0, 1,
                 out3, ws)
        ctx.save_for_backward(buf)
        ctx.shape = (x.shape, V)
        return out3[0]

    @staticmethod
    def backward(ctx, g):
        (buf,) = ctx.saved_tensors
        shape, V = ctx.shape
        src = buf[:, :V].contiguous()
        out = torch.empty_like(src)
        hip.call("oe_axpby", src, None, out.numel(), 1.0, 0.0, g.contiguous().view(1), out)
        return out.view(shape), None, None, None, None


class EmbedFn(torch.autograd.Function):
    """decoder.py:144-147,186: Embedding -> x*sqrt(d) + pe."""

    @staticmethod
    def forward(ctx, tokens, table, pe, xscale):
        B, L = tokens.shape
        V, d = table.shape
        tok = tokens.to(torch.int64).contiguous()
        out = _new(B, L, d, like=table)
        hip.call("oe_embed_fwd", tok, table, pe, B * L, L, d, V, xscale, out)
        ctx.save_for_backward(tok)
        ctx.table_ref = table
        ctx.cfg = (V, d, xscale)
        return out

    @staticmethod
    def backward(ctx, dout):
        (tok,) = ctx.saved_tensors
        V, d, xscale = ctx.cfg
        dout = dout.contiguous()
        dt, rt = grad_sink(ctx.table_ref)
        hip.call("oe_embed_bwd", tok, dout, tok.numel(), d, V, xscale, dt)
        stamp("bwd: a decoder's backward done")
        return None, rt, None, None


def embed(tokens, table, pe, xscale):
    return EmbedFn.apply(tokens, table, pe, xscale)


# --------------------------------------------------------------------------- #
# inference helpers
# --------------------------------------------------------------------------- #
def ctc_greedy(logits, ldv, B, T, V, hlens, eos):
    fb = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    ot = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    ol = torch.empty(B, dtype=torch.int32, device=logits.device)
    hl = hlens.to(torch.int32).contiguous()
    hip.call("oe_ctc_greedy", logits, ldv, B, T, V, hl, eos, fb, ot, ol)
    return ot, ol


def ctc_align(logits, ldv, B, T, V, hlens, ys, ylens):
    """CTC forced alignment (oe_ctc_align; semantics in include/openeat_hip.h): logits (B, T, ldv) float32, ys (B, Lmax)
    labels of which ylens[b] count -> device tensors (frames (B, T) int32, start (B, Lmax) int32, end (B, Lmax) int32,
    tok_logp (B, Lmax) float32, score (B) float32)."""
    logits = _chk(logits, "ctc_align")
    dev = logits.device
    Lmax = int(ys.shape[1])
    ys32 = ys.to(torch.int32).contiguous()
    if Lmax == 0:                               # the C ABI wants a row per utterance; nothing of it is read
        ys32 = torch.zeros(B, 1, dtype=torch.int32, device=dev)
    Lk = max(Lmax, 1)
    hl32, yl32 = hlens.to(torch.int32).contiguous(), ylens.to(torch.int32).contiguous()
    frames = torch.empty(B, T, dtype=torch.int32, device=dev)
    start = torch.empty(B, Lk, dtype=torch.int32, device=dev)
    end = torch.empty(B, Lk, dtype=torch.int32, device=dev)
    tok_logp = torch.empty(B, Lk, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(hip.lib().oe_ctc_align_workspace_bytes(B, T, Lk), dtype=torch.uint8, device=dev)
    hip.call("oe_ctc_align", logits, ldv, B, T, V, hl32, ys32, Lk, yl32, frames, start, end, tok_logp, score, ws)
    return frames, start[:, :Lmax], end[:, :Lmax], tok_logp[:, :Lmax], score


def ctc_segment(logits, ldv, B, T, V, hlens, ys, ylens, free_start=True, free_end=True):
    """Long-form CTC segmentation (oe_ctc_segment; semantics in include/openeat_hip.h): logits (B, T, ldv) float32 of whole
    recordings, ys (B, Lmax <= 8191) the recordings' concatenated labels of which ylens[b] count; free_start / free_end make
    the audio before / after the transcript free -> device tensors (frames (B, T) int32, path_logp (B, T) float32,
    start (B, Lmax) int32, end (B, Lmax) int32, tok_logp (B, Lmax) float32, score (B) float64)."""
    logits = _chk(logits, "ctc_segment")
    dev = logits.device
    Lmax = int(ys.shape[1])
    ys32 = ys.to(torch.int32).contiguous()
    if Lmax == 0:                               # the C ABI wants a row per recording; nothing of it is read
        ys32 = torch.zeros(B, 1, dtype=torch.int32, device=dev)
    Lk = max(Lmax, 1)
    hl32, yl32 = hlens.to(torch.int32).contiguous(), ylens.to(torch.int32).contiguous()
    frames = torch.empty(B, T, dtype=torch.int32, device=dev)
    path_logp = torch.empty(B, T, dtype=torch.float32, device=dev)
    start = torch.empty(B, Lk, dtype=torch.int32, device=dev)
    end = torch.empty(B, Lk, dtype=torch.int32, device=dev)
    tok_logp = torch.empty(B, Lk, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    nbytes = hip.lib().oe_ctc_segment_workspace_bytes(B, T, V, Lk)
    if nbytes == 0:
        raise ValueError(f"ctc_segment: B={B} T={T} Lmax={Lmax} outside 1 <= B, 1 <= T <= 2^20, Lmax <= 8191")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a = hip.CtcSegmentArgs()
    a.logits, a.ldv, a.B, a.T, a.V = logits.data_ptr(), ldv, B, T, V
    a.hlens, a.targets, a.Lmax, a.tlens = hl32.data_ptr(), ys32.data_ptr(), Lk, yl32.data_ptr()
    a.free_start, a.free_end = int(bool(free_start)), int(bool(free_end))
    a.frames, a.path_logp, a.tok_start, a.tok_end = frames.data_ptr(), path_logp.data_ptr(), start.data_ptr(), end.data_ptr()
    a.tok_logp, a.score, a.workspace = tok_logp.data_ptr(), score.data_ptr(), ws.data_ptr()
    hip.check(hip.lib().oe_ctc_segment(hip.C.byref(a), hip.stream()), "oe_ctc_segment")
    return frames, path_logp, start[:, :Lmax], end[:, :Lmax], tok_logp[:, :Lmax], score


def ctc_keyword_search(logits, hlens, keywords, max_hits=8, normalized=False, max_workspace_bytes=1 << 30):
    """Keyword search over CTC posteriors (oe_ctc_kws; semantics in include/openeat_hip.h): logits (B, T, V) float32 (raw, or
    log-probabilities with normalized=True), hlens (B), keywords an openeat_amd.utils.keyword.KeywordList -> device tensors
    (n_hits (B, K) int32, hit_start, hit_end (B, K, max_hits) int32, hit_score (B, K, max_hits) float32, best_start, best_end
    (B, K) int32, best_score (B, K) float32).  The workspace is B * T * (U + 1) floats for the U distinct tokens of the list;
    where that exceeds max_workspace_bytes the keywords - they are independent - run in consecutive groups of at most as many
    distinct tokens as fit, one workspace reused, and the results are concatenated: exactly those of one call."""
    from openeat_amd.utils.keyword import KeywordList
    if not isinstance(keywords, KeywordList):
        raise TypeError(f"ctc_keyword_search: keywords must be an openeat_amd.utils.keyword.KeywordList (got {type(keywords).__name__})")
    logits = _chk(logits, "ctc_keyword_search")
    if logits.dim() != 3:
        raise ValueError(f"ctc_keyword_search: logits must be (B, T, V), got {tuple(logits.shape)}")
    B, T, V = logits.shape
    dev = logits.device
    K, max_hits = len(keywords), int(max_hits)
    if B < 1 or not 1 <= T <= 1 << 20 or max_hits < 1 or len(keywords.cols) >= V:
        raise ValueError(f"ctc_keyword_search: B={B} T={T} max_hits={max_hits} U={len(keywords.cols)} V={V} outside 1 <= B, "
                         "1 <= T <= 2^20, 1 <= max_hits, U < V")
    hl32 = hlens.to(device=dev, dtype=torch.int32).contiguous()
    max_cols = max(int(max_workspace_bytes) // (4 * B * T) - 1, 1)
    bounds = keywords.group_bounds(max_cols) if len(keywords.cols) > max_cols else [0, K]
    n_hits = torch.empty(B, K, dtype=torch.int32, device=dev)
    hit_start = torch.empty(B, K, max_hits, dtype=torch.int32, device=dev)
    hit_end = torch.empty(B, K, max_hits, dtype=torch.int32, device=dev)
    hit_score = torch.empty(B, K, max_hits, dtype=torch.float32, device=dev)
    best_start = torch.empty(B, K, dtype=torch.int32, device=dev)
    best_end = torch.empty(B, K, dtype=torch.int32, device=dev)
    best_score = torch.empty(B, K, dtype=torch.float32, device=dev)
    outs = (n_hits, hit_start, hit_end, hit_score, best_start, best_end, best_score)
    groups = [keywords] if len(bounds) == 2 else [keywords.subset(lo, hi) for lo, hi in zip(bounds, bounds[1:])]
    ws = torch.empty(max(hip.lib().oe_ctc_kws_workspace_bytes(B, T, len(g.cols)) for g in groups), dtype=torch.uint8, device=dev)
    for g, lo, hi in zip(groups, bounds, bounds[1:]):
        # one group: its own outputs (B, hi - lo, ..) - a slice of the full ones is not dense unless B == 1 or the group is all
        part = outs if len(groups) == 1 else tuple(o.new_empty((B, hi - lo) + tuple(o.shape[2:])) for o in outs)
        a = hip.CtcKwsArgs()
        a.logits, a.ldv, a.B, a.T, a.V = logits.data_ptr(), V, B, T, V
        a.hlens, a.kws = hl32.data_ptr(), hip.C.pointer(hip.keyword_set(g, dev))
        a.normalized, a.max_hits = int(bool(normalized)), max_hits
        a.n_hits, a.hit_start, a.hit_end, a.hit_score = (t.data_ptr() for t in part[:4])
        a.best_start, a.best_end, a.best_score = (t.data_ptr() for t in part[4:])
        a.workspace = ws.data_ptr()
        hip.check(hip.lib().oe_ctc_kws(hip.C.byref(a), hip.stream()), "oe_ctc_kws")
        if part is not outs:
            for o, q in zip(outs, part):
                o[:, lo:hi] = q
    return outs


def _graph_decode_front(name, logits, hlens, graph):
    """What the graph decoders' wrappers do first: graph's type, logits (B, T, V) float32 on the device and contiguous ->
    (logits, hl32, (B, T, V), (U, Q, A))."""
    from openeat_amd.utils.decoding_graph import DecodingGraph
    if not isinstance(graph, DecodingGraph):
        raise TypeError(f"{name}: graph must be an openeat_amd.utils.decoding_graph.DecodingGraph (got {type(graph).__name__})")
    logits = _chk(logits, name)
    if logits.dim() != 3:
        raise ValueError(f"{name}: logits must be (B, T, V), got {tuple(logits.shape)}")
    logits = logits.contiguous()
    hl32 = hlens.to(device=logits.device, dtype=torch.int32).contiguous()
    return logits, hl32, tuple(logits.shape), (len(graph.cols), graph.num_nodes, graph.num_arcs)


def _graph_decode_groups(make_args, logits, hl32, g, ws, group):
    """The utterances in consecutive groups of at most `group`: (args, lo) per group, args with the fields every graph decoder
    has filled in for the utterances lo .. lo+n-1 (those rows of every (B, ..) tensor are dense), one workspace reused."""
    B, T, V = logits.shape
    for lo in range(0, B, group):
        a = make_args()
        a.logits, a.ldv, a.B, a.T, a.V = logits[lo].data_ptr(), V, min(group, B - lo), T, V
        a.hlens, a.graph, a.workspace = hl32[lo:].data_ptr(), hip.C.pointer(g), ws.data_ptr()
        yield a, lo


def ctc_graph_decode(logits, hlens, graph, normalized=False, max_trav=None, workspace_cap=1 << 30):
    """Grammar-constrained CTC decoding (oe_ctc_graph; semantics in include/openeat_hip.h): logits (B, T, V) float32 (raw, or
    log-probabilities with normalized=True), hlens (B), graph an openeat_amd.utils.decoding_graph.DecodingGraph -> device
    tensors (score (B) float32, frames, arcs (B, T) int32, path_logp (B, T) float32, n_trav (B) int32, trav_arc, trav_start,
    trav_end (B, max_trav) int32, trav_logp (B, max_trav) float32).  max_trav None: T, which no path exceeds.  The workspace
    is 4 * T * (U + 1 + Q + ceil(A / 4)) bytes per utterance; where that exceeds workspace_cap for the batch the utterances -
    they are independent - run in consecutive groups of as many as fit (at least one), one workspace reused: exactly the
    results of one call."""
    logits, hl32, (B, T, V), (U, Q, A) = _graph_decode_front("ctc_graph_decode", logits, hlens, graph)
    dev = logits.device
    max_trav = T if max_trav is None else int(max_trav)
    per_utt = hip.lib().oe_ctc_graph_workspace_bytes(1, T, U, Q, A) if B >= 1 else 0
    if per_utt == 0 or max_trav < 1 or U >= V:
        raise ValueError(f"ctc_graph_decode: B={B} T={T} max_trav={max_trav} U={U} V={V} Q={Q} A={A} outside 1 <= B, 1 <= T <= 2^20, "
                         "1 <= max_trav, 1 <= U < V, 1 <= Q <= 8064, 1 <= A <= 16384 (a graph without arcs has no device form)")
    score = torch.empty(B, dtype=torch.float32, device=dev)
    frames = torch.empty(B, T, dtype=torch.int32, device=dev)
    arcs = torch.empty(B, T, dtype=torch.int32, device=dev)
    path_logp = torch.empty(B, T, dtype=torch.float32, device=dev)
    n_trav = torch.empty(B, dtype=torch.int32, device=dev)
    trav_arc = torch.empty(B, max_trav, dtype=torch.int32, device=dev)
    trav_start = torch.empty(B, max_trav, dtype=torch.int32, device=dev)
    trav_end = torch.empty(B, max_trav, dtype=torch.int32, device=dev)
    trav_logp = torch.empty(B, max_trav, dtype=torch.float32, device=dev)
    outs = (score, frames, arcs, path_logp, n_trav, trav_arc, trav_start, trav_end, trav_logp)
    group = min(max(int(workspace_cap) // per_utt, 1), B)
    ws = torch.empty(per_utt * group, dtype=torch.uint8, device=dev)
    for a, lo in _graph_decode_groups(hip.CtcGraphArgs, logits, hl32, hip.decoding_graph(graph, dev), ws, group):
        a.normalized, a.max_trav = int(bool(normalized)), max_trav
        a.score, a.frames, a.arcs, a.path_logp = (t[lo:].data_ptr() for t in outs[:4])
        a.n_trav, a.trav_arc, a.trav_start, a.trav_end, a.trav_logp = (t[lo:].data_ptr() for t in outs[4:])
        hip.check(hip.lib().oe_ctc_graph(hip.C.byref(a), hip.stream()), "oe_ctc_graph")
    return outs


def ctc_graph_nbest(logits, hlens, graph, nbest, distinct="arcs", normalized=False, max_len=None, workspace_cap=1 << 30):
    """N-best grammar-constrained CTC decoding (oe_ctc_graph_nbest; semantics in include/openeat_hip.h): logits (B, T, V)
    float32 (raw, or log-probabilities with normalized=True), hlens (B), graph an
    openeat_amd.utils.decoding_graph.DecodingGraph, 1 <= nbest <= 8, distinct "arcs" (distinct paths) or "tokens" (distinct
    token sequences, each with its best path) -> device tensors (n_hyp (B) int32, hyp_score (B, nbest) float32, hyp_len
    (B, nbest) int32, hyp_arcs, hyp_tokens (B, nbest, max_len) int32).  max_len None: T, which no path exceeds.  The workspace
    is dominated by the record table, 4 * T * A * nbest bytes per utterance; where the batch exceeds workspace_cap the
    utterances - they are independent - run in consecutive groups of as many as fit, one workspace reused: exactly the results
    of one call.  One utterance alone above the cap is a ValueError that names the bytes."""
    logits, hl32, (B, T, V), (U, Q, A) = _graph_decode_front("ctc_graph_nbest", logits, hlens, graph)
    modes = {"arcs": hip.CTC_GRAPH_NBEST_ARCS, "tokens": hip.CTC_GRAPH_NBEST_TOKENS}
    if distinct not in modes:
        raise ValueError(f"ctc_graph_nbest: distinct is 'arcs' or 'tokens', got {distinct!r}")
    dev = logits.device
    nbest = int(nbest)
    max_len = T if max_len is None else int(max_len)
    lib = hip.lib()
    per_utt = lib.oe_ctc_graph_nbest_workspace_bytes(1, T, U, Q, A, nbest) if B >= 1 else 0
    if per_utt == 0 or max_len < 1 or U >= V:
        raise ValueError(f"ctc_graph_nbest: B={B} T={T} nbest={nbest} max_len={max_len} U={U} V={V} Q={Q} A={A} outside 1 <= B, "
                         "1 <= T <= 2^20, 1 <= nbest <= 8, 1 <= max_len, 1 <= U < V, 1 <= Q <= 8064, 1 <= A <= 16384, T*A*nbest < 2^31")
    if per_utt > int(workspace_cap):
        raise ValueError(f"ctc_graph_nbest: one utterance needs a workspace of {per_utt} bytes (T={T} A={A} nbest={nbest}: the record "
                         f"table alone is {4 * T * A * nbest}), above workspace_cap={int(workspace_cap)}")
    n_hyp = torch.empty(B, dtype=torch.int32, device=dev)
    hyp_score = torch.empty(B, nbest, dtype=torch.float32, device=dev)
    hyp_len = torch.empty(B, nbest, dtype=torch.int32, device=dev)
    hyp_arcs = torch.empty(B, nbest, max_len, dtype=torch.int32, device=dev)
    hyp_tokens = torch.empty(B, nbest, max_len, dtype=torch.int32, device=dev)
    outs = (n_hyp, hyp_score, hyp_len, hyp_arcs, hyp_tokens)
    group = min(int(workspace_cap) // per_utt, B)
    ws = torch.empty(lib.oe_ctc_graph_nbest_workspace_bytes(group, T, U, Q, A, nbest), dtype=torch.uint8, device=dev)
    for a, lo in _graph_decode_groups(hip.CtcGraphNbestArgs, logits, hl32, hip.decoding_graph(graph, dev), ws, group):
        a.normalized, a.nbest, a.distinct, a.max_len = int(bool(normalized)), nbest, modes[distinct], max_len
        a.n_hyp, a.hyp_score, a.hyp_len, a.hyp_arcs, a.hyp_tokens = (t[lo:].data_ptr() for t in outs)
        hip.check(lib.oe_ctc_graph_nbest(hip.C.byref(a), hip.stream()), "oe_ctc_graph_nbest")
    return outs


def ctc_graph_beam_decode(logits, hlens, graph, beam, max_active=16384, normalized=False, max_trav=None, workspace_cap=1 << 30):
    """Beam-pruned CTC decoding over a large token graph (oe_ctc_graph_beam; semantics in include/openeat_hip.h): logits
    (B, T, V) float32 (raw, or log-probabilities with normalized=True), hlens (B), graph an
    openeat_amd.utils.decoding_graph.DecodingGraph of either size, beam >= 0 or inf, max_active the survivors a frame can
    record -> ctc_graph_decode's device tensors and status (B) int32 (0 decoded, 1 infeasible, 2 overflow: more than
    max_active survivors in some frame) and peak (B) int32 (the largest survivor count, on overflow the overflowing one).
    The workspace is 4 * T * (U + 1) bytes of rows and 40 Q + 20 A + (28 + 8 T) min(max_active, Q + A) bytes of state per
    utterance; where that exceeds workspace_cap for the batch the utterances run in consecutive groups of as many as fit (at
    least one), one workspace reused: exactly the results of one call.  No host read."""
    logits, hl32, (B, T, V), (U, Q, A) = _graph_decode_front("ctc_graph_beam_decode", logits, hlens, graph)
    dev = logits.device
    max_trav = T if max_trav is None else int(max_trav)
    beam, max_active = float(beam), int(max_active)
    lib = hip.lib()
    per_utt = lib.oe_ctc_graph_beam_workspace_bytes(1, T, U, Q, A, max_active) if B >= 1 and 1 <= max_active < 1 << 31 else 0
    if per_utt == 0 or max_trav < 1 or U >= V or not beam >= 0:
        raise ValueError(f"ctc_graph_beam_decode: B={B} T={T} max_trav={max_trav} max_active={max_active} beam={beam} U={U} V={V} Q={Q} "
                         f"A={A} outside 1 <= B, 1 <= T <= 2^20, 1 <= max_trav, 1 <= max_active, 0 <= beam, 1 <= U < V, 1 <= Q <= 2^20, "
                         "1 <= A <= 2^22 (a graph without arcs has no device form)")
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    outs = (f32(B), i32(B, T), i32(B, T), f32(B, T), i32(B), i32(B, max_trav), i32(B, max_trav), i32(B, max_trav), f32(B, max_trav),
            i32(B), i32(B))
    group = min(max(int(workspace_cap) // per_utt, 1), B)
    ws = torch.empty(lib.oe_ctc_graph_beam_workspace_bytes(group, T, U, Q, A, max_active), dtype=torch.uint8, device=dev)
    for a, lo in _graph_decode_groups(hip.CtcGraphBeamArgs, logits, hl32, hip.beam_graph(graph, dev), ws, group):
        a.normalized, a.max_trav, a.max_active, a.beam = int(bool(normalized)), max_trav, max_active, beam
        a.score, a.frames, a.arcs, a.path_logp = (t[lo:].data_ptr() for t in outs[:4])
        a.n_trav, a.trav_arc, a.trav_start, a.trav_end, a.trav_logp = (t[lo:].data_ptr() for t in outs[4:9])
        a.status, a.peak = outs[9][lo:].data_ptr(), outs[10][lo:].data_ptr()
        hip.check(lib.oe_ctc_graph_beam(hip.C.byref(a), hip.stream()), "oe_ctc_graph_beam")
    return outs


class CTCGraphLogpFn(torch.autograd.Function):
    """oe_ctc_graph_logp / oe_ctc_graph_logp_grad (semantics in include/openeat_hip.h): the total log-likelihood of a decoding
    graph per utterance, differentiable with respect to raw logits.  The utterances run in consecutive groups under the
    workspace cap, forward and backward, one workspace reused: exactly the results of one call."""

    @staticmethod
    def forward(ctx, logits, hl32, gset, graph_of, normalized, cap):
        B, T, V = (int(s) for s in logits.shape)
        # rows padded beyond V (CTCHeadFn's logits, a [..., :V] view of them) are taken as they are
        if logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == T * logits.stride(1) and logits.data_ptr() % 4 == 0:
            buf, ld = logits, int(logits.stride(1))
        else:
            buf, ld = logits.contiguous(), V
        dev = logits.device
        lib = hip.lib()
        U, Qmax, Amax = len(gset.cols), gset.Qmax, gset.Amax
        per_utt = lib.oe_ctc_graph_logp_workspace_bytes(1, T, U, Qmax, Amax)
        if per_utt == 0 or U >= V:
            raise ValueError(f"ctc_graph_logp: T={T} U={U} V={V} Qmax={Qmax} Amax={Amax} outside 1 <= T <= 2^20, 1 <= U < V, "
                             f"Qmax <= {gset.MAX_NODES}, 1 <= Amax <= {gset.MAX_ARCS}")
        gs = hip.graph_set(gset, dev)
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        group = min(max(int(cap) // per_utt, 1), B)
        ws = torch.empty(per_utt * group + 16, dtype=torch.uint8, device=dev)
        for lo in range(0, B, group):
            a = hip.CtcGraphLogpArgs()
            a.logits, a.ldv, a.B, a.T, a.V = buf.data_ptr() + 4 * lo * T * ld, ld, min(group, B - lo), T, V
            a.hlens, a.set = hl32[lo:].data_ptr(), hip.C.pointer(gs)
            a.graph_of = None if graph_of is None else graph_of[lo:].data_ptr()
            a.normalized, a.logp, a.workspace = int(bool(normalized)), logp[lo:].data_ptr(), ws.data_ptr()
            hip.check(lib.oe_ctc_graph_logp(hip.C.byref(a), hip.stream()), "oe_ctc_graph_logp")
        if ctx.needs_input_grad[0]:
            if normalized:
                raise ValueError("ctc_graph_logp: the gradient is with respect to raw logits (normalized=False)")
            ctx.save_for_backward(buf, hl32, *(() if graph_of is None else (graph_of,)))
            ctx.cfg = (B, T, V, ld, gset, int(cap))
        return logp

    @staticmethod
    def backward(ctx, g):
        buf, hl32, *rest = ctx.saved_tensors
        graph_of = rest[0] if rest else None
        B, T, V, ld, gset, cap = ctx.cfg
        g = _chk(g, "ctc_graph_logp gradient")
        dev = buf.device
        lib = hip.lib()
        per_utt = lib.oe_ctc_graph_logp_grad_workspace_bytes(1, T, len(gset.cols), gset.Qmax, gset.Amax)
        gs = hip.graph_set(gset, dev)
        dlogits = torch.empty(B, T, ld, dtype=torch.float32, device=dev)
        group = min(max(cap // per_utt, 1), B)
        ws = torch.empty(lib.oe_ctc_graph_logp_grad_workspace_bytes(group, T, len(gset.cols), gset.Qmax, gset.Amax), dtype=torch.uint8, device=dev)
        for lo in range(0, B, group):
            a = hip.CtcGraphLogpGradArgs()
            a.logits, a.ldv, a.B, a.T, a.V = buf.data_ptr() + 4 * lo * T * ld, ld, min(group, B - lo), T, V
            a.hlens, a.set = hl32[lo:].data_ptr(), hip.C.pointer(gs)
            a.graph_of = None if graph_of is None else graph_of[lo:].data_ptr()
            a.normalized, a.g, a.dlogits, a.logp, a.workspace = 0, g[lo:].data_ptr(), dlogits[lo].data_ptr(), None, ws.data_ptr()
            hip.check(lib.oe_ctc_graph_logp_grad(hip.C.byref(a), hip.stream()), "oe_ctc_graph_logp_grad")
        return dlogits[..., :V], None, None, None, None, None


def ctc_graph_logp(logits, hlens, graphs, graph_of=None, normalized=False, workspace_cap=1 << 30):
    """The total log-likelihood of a decoding graph (oe_ctc_graph_logp; semantics in include/openeat_hip.h): logits (B, T, V)
    float32 (raw, or log-probabilities with normalized=True), hlens (B), graphs a DecodingGraph, a list of them or a GraphSet
    (openeat_amd.utils.decoding_graph), graph_of (B) the graph of each utterance (None: graph 0 for all) -> logp (B) float32,
    -inf for an infeasible utterance.  Differentiable with respect to raw logits (an infeasible utterance takes a zero
    gradient); padded-row views are taken as CTCNbestFn takes them.  Where the workspace exceeds workspace_cap the utterances
    run in consecutive groups, one workspace reused, forward and backward: exactly the results of one call.  No host read."""
    from openeat_amd.utils.decoding_graph import DecodingGraph, GraphSet
    if isinstance(graphs, DecodingGraph) or (isinstance(graphs, (list, tuple)) and all(isinstance(x, DecodingGraph) for x in graphs)):
        graphs = GraphSet(graphs)
    if not isinstance(graphs, GraphSet):
        raise TypeError(f"ctc_graph_logp: graphs must be a DecodingGraph, a list of them or a GraphSet (got {type(graphs).__name__})")
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3):
        raise TypeError("ctc_graph_logp: logits must be a float32 (B, T, V) CUDA tensor; there is no CPU fallback")
    pend = _PENDING_LNF.take(logits)
    if pend is not None:
        pend.resolve()
    B = int(logits.shape[0])
    if B < 1 or tuple(hlens.shape) != (B,):
        raise ValueError(f"ctc_graph_logp: B={B} utterances need hlens (B), got {tuple(hlens.shape)}")
    dev = logits.device
    hl32 = hlens.to(device=dev, dtype=torch.int32).contiguous()
    if graph_of is not None:
        graph_of = torch.as_tensor(graph_of).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(graph_of.shape) != (B,):
            raise ValueError(f"ctc_graph_logp: graph_of must be (B,) = ({B},), got {tuple(graph_of.shape)}")
    return CTCGraphLogpFn.apply(logits, hl32, graphs, graph_of, bool(normalized), int(workspace_cap))


class CTCGraphBeamLogpFn(torch.autograd.Function):
    """oe_ctc_graph_beam_logp / oe_ctc_graph_beam_logp_grad (semantics in include/openeat_hip.h): the beam-pruned total
    log-likelihood of a decoding graph of any size per utterance, differentiable with respect to raw logits.  The utterances
    run in consecutive groups under the workspace cap, forward and backward, one workspace reused: exactly the results of one
    call."""

    @staticmethod
    def _fill(a, buf, ld, hl32, g, lo, n, T, V, beam, max_active, normalized, ws):
        a.logits, a.ldv, a.B, a.T, a.V = buf.data_ptr() + 4 * lo * T * ld, ld, n, T, V
        a.hlens, a.graph, a.workspace = hl32[lo:].data_ptr(), hip.C.pointer(g), ws.data_ptr()
        a.normalized, a.max_active, a.beam = int(bool(normalized)), max_active, beam

    @staticmethod
    def forward(ctx, logits, hl32, graph, beam, max_active, normalized, cap):
        B, T, V = (int(s) for s in logits.shape)
        # rows padded beyond V (CTCHeadFn's logits, a [..., :V] view of them) are taken as they are
        if logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == T * logits.stride(1) and logits.data_ptr() % 4 == 0:
            buf, ld = logits, int(logits.stride(1))
        else:
            buf, ld = logits.contiguous(), V
        dev = logits.device
        lib = hip.lib()
        U, Q, A = len(graph.cols), graph.num_nodes, graph.num_arcs
        per_utt = lib.oe_ctc_graph_beam_logp_workspace_bytes(1, T, U, Q, A, max_active) if 1 <= max_active < 1 << 31 else 0
        if per_utt == 0 or U >= V or not beam >= 0:
            raise ValueError(f"ctc_graph_beam_logp: T={T} max_active={max_active} beam={beam} U={U} V={V} Q={Q} A={A} outside 1 <= T <= 2^20, "
                             "1 <= max_active, 0 <= beam, 1 <= U < V, 1 <= Q <= 2^20, 1 <= A <= 2^22 (a graph without arcs has no device "
                             "form)")
        g = hip.beam_logp_graph(graph, dev)
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        peak = torch.empty(B, dtype=torch.int32, device=dev)
        group = min(max(int(cap) // per_utt, 1), B)
        ws = torch.empty(lib.oe_ctc_graph_beam_logp_workspace_bytes(group, T, U, Q, A, max_active), dtype=torch.uint8, device=dev)
        for lo in range(0, B, group):
            a = hip.CtcGraphBeamLogpArgs()
            CTCGraphBeamLogpFn._fill(a, buf, ld, hl32, g, lo, min(group, B - lo), T, V, beam, max_active, normalized, ws)
            a.logp, a.status, a.peak = logp[lo:].data_ptr(), status[lo:].data_ptr(), peak[lo:].data_ptr()
            hip.check(lib.oe_ctc_graph_beam_logp(hip.C.byref(a), hip.stream()), "oe_ctc_graph_beam_logp")
        if ctx.needs_input_grad[0]:
            if normalized:
                raise ValueError("ctc_graph_beam_logp: the gradient is with respect to raw logits (normalized=False)")
            ctx.save_for_backward(buf, hl32)
            ctx.cfg = (B, T, V, ld, graph, beam, max_active, int(cap))
        ctx.mark_non_differentiable(status, peak)
        return logp, status, peak

    @staticmethod
    def backward(ctx, g, _status, _peak):
        buf, hl32 = ctx.saved_tensors
        B, T, V, ld, graph, beam, max_active, cap = ctx.cfg
        g = _chk(g, "ctc_graph_beam_logp gradient")
        dev = buf.device
        lib = hip.lib()
        U, Q, A = len(graph.cols), graph.num_nodes, graph.num_arcs
        per_utt = lib.oe_ctc_graph_beam_logp_grad_workspace_bytes(1, T, U, Q, A, max_active)
        gr = hip.beam_logp_graph(graph, dev)
        dlogits = torch.empty(B, T, ld, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        peak = torch.empty(B, dtype=torch.int32, device=dev)
        group = min(max(cap // per_utt, 1), B)
        ws = torch.empty(lib.oe_ctc_graph_beam_logp_grad_workspace_bytes(group, T, U, Q, A, max_active), dtype=torch.uint8, device=dev)
        for lo in range(0, B, group):
            a = hip.CtcGraphBeamLogpGradArgs()
            CTCGraphBeamLogpFn._fill(a, buf, ld, hl32, gr, lo, min(group, B - lo), T, V, beam, max_active, False, ws)
            a.g, a.dlogits, a.logp = g[lo:].data_ptr(), dlogits[lo].data_ptr(), None
            a.status, a.peak = status[lo:].data_ptr(), peak[lo:].data_ptr()
            hip.check(lib.oe_ctc_graph_beam_logp_grad(hip.C.byref(a), hip.stream()), "oe_ctc_graph_beam_logp_grad")
        return dlogits[..., :V], None, None, None, None, None, None


def ctc_graph_beam_logp(logits, hlens, graph, beam, max_active=16384, normalized=False, workspace_cap=1 << 30):
    """The beam-pruned total log-likelihood of a decoding graph of any size (oe_ctc_graph_beam_logp; semantics in
    include/openeat_hip.h): logits (B, T, V) float32 (raw, or log-probabilities with normalized=True), hlens (B), graph an
    openeat_amd.utils.decoding_graph.DecodingGraph, beam >= 0 or inf, max_active the survivors a frame can record ->
    (logp (B) float32, -inf for an infeasible or overflowed utterance; status (B) int32: 0 summed, 1 infeasible, 2 overflow;
    peak (B) int32: the largest survivor count, on overflow the overflowing one).  logp is differentiable with respect to raw
    logits, the survivor sets held fixed (an infeasible or overflowed utterance takes a zero gradient); padded-row views are
    taken as CTCNbestFn takes them.  Where the workspace exceeds workspace_cap the utterances run in consecutive groups, one
    workspace reused, forward and backward: exactly the results of one call.  No host read."""
    from openeat_amd.utils.decoding_graph import DecodingGraph
    if not isinstance(graph, DecodingGraph):
        raise TypeError(f"ctc_graph_beam_logp: graph must be an openeat_amd.utils.decoding_graph.DecodingGraph (got {type(graph).__name__})")
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3):
        raise TypeError("ctc_graph_beam_logp: logits must be a float32 (B, T, V) CUDA tensor; there is no CPU fallback")
    pend = _PENDING_LNF.take(logits)
    if pend is not None:
        pend.resolve()
    B = int(logits.shape[0])
    if B < 1 or tuple(hlens.shape) != (B,):
        raise ValueError(f"ctc_graph_beam_logp: B={B} utterances need hlens (B), got {tuple(hlens.shape)}")
    hl32 = hlens.to(device=logits.device, dtype=torch.int32).contiguous()
    return CTCGraphBeamLogpFn.apply(logits, hl32, graph, float(beam), int(max_active), bool(normalized), int(workspace_cap))


def ngram_score(lm, tokens, lens, bos: bool = True, eos: bool = True, per_token: bool = False):
    """Back-off n-gram LM scores of R hypotheses (oe_ngram_score; asr_model.py:515-516 for all of them at once): `lm` an
    openeat_amd.models.ngram_lm.NgramLM, tokens (R, ld) integer token ids and lens (R) on the device (a negative length:
    the slot does not exist, score -inf; what lies behind a length is not read) -> score (R) float64, total log10
    probability.  per_token: also (tok_logp (R, ld+1) float64, tok_order (R, ld+1) int32), zero where nothing is written.
    No host read, no allocation beyond the outputs: capturable."""
    if not (isinstance(tokens, torch.Tensor) and isinstance(lens, torch.Tensor) and tokens.is_cuda and lens.is_cuda):
        raise TypeError("ngram_score: openeat_amd ops need CUDA tensors; there is no CPU fallback (on the host: NgramLM.score)")
    if tokens.dtype.is_floating_point or lens.dtype.is_floating_point or tokens.dim() != 2 or lens.shape != tokens.shape[:1]:
        raise TypeError("ngram_score: tokens (R, ld) and lens (R) must be integer tensors")
    dev = tokens.device
    R, ld = int(tokens.shape[0]), int(tokens.shape[1])
    tok32 = tokens.to(torch.int32).contiguous()
    len32 = lens.to(torch.int32).contiguous()
    score = torch.empty(R, dtype=torch.float64, device=dev)
    tok_logp = torch.zeros(R, ld + 1, dtype=torch.float64, device=dev) if per_token else None
    tok_order = torch.zeros(R, ld + 1, dtype=torch.int32, device=dev) if per_token else None
    hip.call("oe_ngram_score", hip.ngram_model(lm, dev), tok32, ld, len32, R, int(bool(bos)), int(bool(eos)), score, tok_logp, tok_order)
    return (score, tok_logp, tok_order) if per_token else score


def ngram_next(lm, tokens, lens, cand=None, eos=None):
    """The n-gram LM term of candidate next tokens of R growing hypotheses (oe_ngram_next; semantics in
    include/openeat_hip.h): `lm` an openeat_amd.models.ngram_lm.NgramLM, tokens (R, ld) integer token ids (after <sos>) and
    lens (R) on the device (a negative length: the slot does not exist, its row is -inf; what lies behind a length is not
    read), cand (R, C) integer token ids or None = every token of the LM's V, eos the token id whose word is </s> (None: no
    token is) -> (R, C) or (R, V) float64 log10 p(candidate | hypothesis), the bits of ngram_score's tok_logp.
    No host read, no allocation beyond the output: capturable."""
    ts = (tokens, lens) if cand is None else (tokens, lens, cand)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise TypeError("ngram_next: openeat_amd ops need CUDA tensors; there is no CPU fallback (on the host: NgramLM.full_scores)")
    if any(t.dtype.is_floating_point or t.dtype == torch.bool for t in ts) or tokens.dim() != 2 or lens.shape != tokens.shape[:1] \
            or (cand is not None and (cand.dim() != 2 or cand.shape[0] != tokens.shape[0])):
        raise TypeError("ngram_next: tokens (R, ld), lens (R) and cand (R, C) must be integer tensors")
    dev = tokens.device
    R, ld = int(tokens.shape[0]), int(tokens.shape[1])
    V = int(lm.tok2word.shape[0])
    C = V if cand is None else int(cand.shape[1])
    if C < 1:
        raise ValueError("ngram_next: cand (R, C) needs at least one candidate per hypothesis")
    eos = -1 if eos is None else int(eos)
    if not -1 <= eos < V:
        raise ValueError(f"ngram_next: eos {eos} is outside the LM's 0..{V - 1}")
    # a zero-width matrix has no storage to point at: nothing of the stand-in is read
    tok32 = tokens.to(torch.int32).contiguous() if ld else torch.zeros(max(R, 1), dtype=torch.int32, device=dev)
    out = torch.empty(R, C, dtype=torch.float64, device=dev)
    if R == 0:
        return out
    hip.call("oe_ngram_next", hip.ngram_model(lm, dev), tok32, ld, lens.to(torch.int32).contiguous(), R,
             None if cand is None else cand.to(torch.int32).contiguous(), C, eos, out)
    return out


def context_next(graph, state, hits, cand=None, eos=None, V=None, want_state: bool = True):
    """The hotword bias of candidate next tokens of R growing hypotheses (oe_context_next; semantics in
    include/openeat_hip.h): `graph` an openeat_amd.utils.context_graph.ContextGraph, state (R) integer automaton states (0: the
    root; outside the graph's states: the slot does not exist, its row is -1 / -inf) and hits (R) float64 on the device,
    cand (R, C) integer token ids or None = every token of a vocabulary of V (required then), eos the token id that ends a
    hypothesis (None: no token does) -> (state' (R, C) int32, hits' (R, C) float64, bias' (R, C) float64), the bits of
    ContextGraph.bias of the extended prefix; want_state=False: bias' alone.
    No host read, no allocation beyond the outputs: capturable."""
    from openeat_amd.utils.context_graph import ContextGraph
    if not isinstance(graph, ContextGraph):
        raise TypeError(f"context_next: graph must be an openeat_amd.utils.context_graph.ContextGraph (got {type(graph).__name__})")
    ts = (state, hits) if cand is None else (state, hits, cand)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise TypeError("context_next: openeat_amd ops need CUDA tensors; there is no CPU fallback (on the host: ContextGraph.bias)")
    ints = (state,) if cand is None else (state, cand)
    if any(t.dtype.is_floating_point or t.dtype == torch.bool for t in ints) or hits.dtype != torch.float64 or state.dim() != 1 \
            or hits.shape != state.shape or (cand is not None and (cand.dim() != 2 or cand.shape[0] != state.shape[0])):
        raise TypeError("context_next: state (R) and cand (R, C) must be integer tensors, hits (R) a float64 tensor")
    if cand is None and V is None:
        raise ValueError("context_next: without cand every token is a candidate: V, the vocabulary size, is required")
    dev = state.device
    R = int(state.shape[0])
    C = int(V) if cand is None else int(cand.shape[1])
    if C < 1:
        raise ValueError("context_next: at least one candidate per hypothesis (cand (R, C) with C >= 1, or V >= 1)")
    eos = -1 if eos is None else int(eos)
    if eos < -1:
        raise ValueError(f"context_next: eos {eos} is no token id (None: no token ends a hypothesis)")
    bias = torch.empty(R, C, dtype=torch.float64, device=dev)
    new_state = torch.empty(R, C, dtype=torch.int32, device=dev) if want_state else None
    new_hits = torch.empty(R, C, dtype=torch.float64, device=dev) if want_state else None
    if R:
        hip.call("oe_context_next", hip.context_graph(graph, dev), state.to(torch.int32).contiguous(), hits.contiguous(), R,
                 None if cand is None else cand.to(torch.int32).contiguous(), C, eos, new_state, new_hits, bias)
    return (new_state, new_hits, bias) if want_state else bias


def edit_distance(ref, ref_lens, hyp, hyp_lens, group: int = 1, align: bool = False):
    """Edit distance of P (reference, hypothesis) pairs on the device (oe_edit_distance; semantics and tie order in
    include/openeat_hip.h): ref (P / group, Nmax) and hyp (P, Mmax) integer token ids, ref_lens (P / group) and hyp_lens (P)
    their lengths, all on the device; pair p compares hyp row p with ref row p // group.  What lies behind a length is not
    read into the result; hyp_lens[p] < 0: the slot does not exist, its row is all -1.  -> counts (P, 4) int32 = cor, sub,
    del, ins; align: also ref_to_hyp (P, Nmax) int32, the hypothesis position of each reference token (-1: deleted or
    beyond the length).  No host read: capturable."""
    ts = (ref, ref_lens, hyp, hyp_lens)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise TypeError("edit_distance: openeat_amd ops need CUDA tensors; there is no CPU fallback")
    if any(t.dtype.is_floating_point or t.dtype == torch.bool for t in ts) or ref.dim() != 2 or hyp.dim() != 2 \
            or ref_lens.shape != ref.shape[:1] or hyp_lens.shape != hyp.shape[:1]:
        raise TypeError("edit_distance: ref (P / group, Nmax), hyp (P, Mmax) and their lengths must be integer tensors")
    dev = hyp.device
    P, Mmax, Nmax = int(hyp.shape[0]), int(hyp.shape[1]), int(ref.shape[1])
    group = int(group)
    if group < 1 or ref.shape[0] * group != P:
        raise ValueError(f"edit_distance: {ref.shape[0]} references x group {group} != {P} hypotheses")
    counts = torch.empty(P, 4, dtype=torch.int32, device=dev)
    r2h = torch.empty(P, Nmax, dtype=torch.int32, device=dev) if align else None
    if P == 0:
        return (counts, r2h) if align else counts
    ref32, hyp32 = ref.to(torch.int32).contiguous(), hyp.to(torch.int32).contiguous()
    ws = None
    if align:
        nbytes = hip.lib().oe_edit_distance_workspace_bytes(P, Nmax, Mmax)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    # a zero-width matrix has no storage to point at: the C ABI takes NULL for it
    hip.call("oe_edit_distance", ref32 if Nmax else None, Nmax, ref_lens.to(torch.int32).contiguous(), group,
             hyp32 if Mmax else None, Mmax, hyp_lens.to(torch.int32).contiguous(), P, Nmax, Mmax, counts,
             r2h if Nmax else None, ws)
    return (counts, r2h) if align else counts


class CTCNbestFn(torch.autograd.Function):
    """oe_ctc_nbest_score / oe_ctc_nbest_grad (semantics in include/openeat_hip.h): the exact CTC log-likelihood of each of
    `group` hypotheses per utterance, differentiable with respect to the logits."""

    @staticmethod
    def forward(ctx, logits, hlens, hyps, hyp_lens, group):
        B, T, V = (int(s) for s in logits.shape)
        Vp = _vpad(V)
        # rows padded to whole float4s, as CTCHeadFn's logits are: a view of such a buffer is taken as it is
        if logits.stride(2) == 1 and logits.stride(1) == Vp and logits.stride(0) == T * Vp and logits.data_ptr() % 16 == 0:
            buf = logits
        else:
            buf = _new(B, T, Vp, like=logits, zero=(Vp != V))
            buf[..., :V].copy_(logits)
        Lmax = int(hyps.shape[1])
        hyp32 = hyps.to(torch.int32).contiguous()
        hl32, len32 = hlens.to(torch.int32).contiguous(), hyp_lens.to(torch.int32).contiguous()
        dev = logits.device
        lib = hip.lib()
        ws = torch.empty(lib.oe_ctc_nbest_workspace_bytes(B, T, group, Lmax), dtype=torch.uint8, device=dev)
        saved = None
        if ctx.needs_input_grad[0]:
            saved = torch.empty(lib.oe_ctc_nbest_saved_bytes(B, T, group, Lmax), dtype=torch.uint8, device=dev)
        logp = _new(B * group, like=logits)
        hip.call("oe_ctc_nbest_score", buf, Vp, B, T, V, hl32, hyp32 if Lmax else None, Lmax, len32, group, Lmax, logp, saved, ws)
        if saved is not None:
            ctx.save_for_backward(buf, hl32, hyp32, len32, logp, saved)
            ctx.cfg = (B, T, V, Vp, group, Lmax)
        return logp.view(B, group)

    @staticmethod
    def backward(ctx, g):
        buf, hl32, hyp32, len32, logp, saved = ctx.saved_tensors
        B, T, V, Vp, group, Lmax = ctx.cfg
        g = _chk(g, "ctc_nbest_logp gradient")
        dlogits = _new(B, T, Vp, like=buf)
        hip.call("oe_ctc_nbest_grad", buf, Vp, B, T, V, hl32, hyp32 if Lmax else None, Lmax, len32, group, Lmax, logp, g, saved,
                 dlogits, None)
        return dlogits[..., :V], None, None, None, None


def ctc_nbest_logp(logits, hlens, hyps, hyp_lens, group: int):
    """Exact CTC log-likelihood of an n-best list: logits (B, T, V) float32 (raw, not normalised), hlens (B) valid frames,
    hyps (B * group, Lmax <= 255) token ids of which hyp_lens (B * group) count (< 0: the slot does not exist), all on the
    device -> logp (B, group) float32, -inf for an infeasible row (the rule is in include/openeat_hip.h).  Differentiable
    with respect to the logits (one launch in backward); hyps and the lengths are not.  No host read: capturable."""
    ts = (logits, hlens, hyps, hyp_lens)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise TypeError("ctc_nbest_logp: openeat_amd ops need CUDA tensors; there is no CPU fallback")
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise TypeError(f"ctc_nbest_logp: logits must be a float32 (B, T, V) tensor (got {logits.dtype}, {tuple(logits.shape)})")
    group = int(group)
    B = int(logits.shape[0])
    if any(t.dtype.is_floating_point or t.dtype == torch.bool for t in ts[1:]) or hyps.dim() != 2 or hlens.shape != (B,) \
            or hyp_lens.shape != hyps.shape[:1]:
        raise TypeError("ctc_nbest_logp: hlens (B), hyps (B * group, Lmax) and hyp_lens (B * group) must be integer tensors")
    if not 1 <= group <= 64 or hyps.shape[0] != B * group:
        raise ValueError(f"ctc_nbest_logp: {B} utterances x group {group} (1..64) != {hyps.shape[0]} hypotheses")
    if hyps.shape[1] > 255:
        raise ValueError(f"ctc_nbest_logp: hypotheses are {hyps.shape[1]} tokens wide; the limit is 255")
    return CTCNbestFn.apply(logits, hlens, hyps, hyp_lens, group)


class RNNTLossFn(torch.autograd.Function):
    """oe_rnnt_loss / oe_rnnt_grad (semantics in include/openeat_hip.h): the transducer log-likelihood per utterance,
    differentiable with respect to the raw joint logits.  Forward: the row pass and the lattice pass; backward: the gradient
    pass over the workspace the forward left - into the logits' own storage when inplace."""

    @staticmethod
    def forward(ctx, logits, hl32, tg32, ul32, blank, inplace):
        B, T, U1, V = (int(s) for s in logits.shape)
        # rows padded beyond V (a [..., :V] view of them) are taken as they are
        ld = int(logits.stride(2))
        if logits.stride(3) == 1 and ld >= V and logits.stride(1) == U1 * ld and logits.stride(0) == T * U1 * ld and logits.data_ptr() % 4 == 0:
            buf = logits
        else:
            buf, ld = logits.contiguous(), V
        lib = hip.lib()
        nbytes = lib.oe_rnnt_workspace_bytes(B, T, U1 - 1)
        if nbytes == 0:
            raise ValueError(f"rnnt_loss: B={B} T={T} U+1={U1} outside 1 <= B, 1 <= T <= 8192, 1 <= U+1 <= 256, B*T*(U+1) < 2^31")
        dev = logits.device
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        a = hip.RnntArgs()
        a.logits, a.ldv, a.B, a.T, a.Umax, a.V = buf.data_ptr(), ld, B, T, U1 - 1, V
        a.hlens, a.targets, a.ulens = hl32.data_ptr(), (tg32.data_ptr() if U1 > 1 else None), ul32.data_ptr()
        a.blank, a.logp, a.status, a.workspace = int(blank), logp.data_ptr(), None, ws.data_ptr()
        hip.check(lib.oe_rnnt_loss(hip.C.byref(a), hip.stream()), "oe_rnnt_loss")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(buf, hl32, tg32, ul32, ws)
            ctx.cfg = (B, T, U1, V, ld, int(blank), bool(inplace))
        return logp

    @staticmethod
    def backward(ctx, g):
        buf, hl32, tg32, ul32, ws = ctx.saved_tensors
        B, T, U1, V, ld, blank, inplace = ctx.cfg
        g = _chk(g, "rnnt_loss gradient")
        dl = buf if inplace else torch.empty_strided(buf.shape, buf.stride(), dtype=torch.float32, device=buf.device)
        a = hip.RnntGradArgs()
        a.logits, a.ldv, a.B, a.T, a.Umax, a.V = buf.data_ptr(), ld, B, T, U1 - 1, V
        a.hlens, a.targets, a.ulens = hl32.data_ptr(), (tg32.data_ptr() if U1 > 1 else None), ul32.data_ptr()
        a.blank, a.g, a.dlogits, a.workspace = blank, g.data_ptr(), dl.data_ptr(), ws.data_ptr()
        hip.check(hip.lib().oe_rnnt_grad(hip.C.byref(a), hip.stream()), "oe_rnnt_grad")
        if inplace:
            torch.autograd.graph.increment_version(buf)      # the logits are gone: whoever saved them for a backward is told so
        return dl, None, None, None, None, None


def rnnt_loss(logits, hlens, targets, ulens, blank: int = 0, inplace: bool = False):
    """The transducer (RNN-T) log-likelihood (oe_rnnt_loss; semantics in include/openeat_hip.h): logits (B, T, U+1, V) float32,
    raw joint outputs; hlens (B) frames, targets (B, U) labels, ulens (B) label counts, int64 or int32 on the device -> logp (B)
    float32.  hlens[b] <= 0, ulens[b] outside 0..U, and a target within the length that is blank or outside 0..V-1 give -inf and
    a zero gradient.  Differentiable with respect to the logits (one launch in backward).  inplace=True writes that gradient
    over the logits' own storage - the largest tensor of a transducer step is then held once, not twice: the logits CANNOT be
    used after backward (their version counter is bumped, so autograd refuses a stale use), and backward runs once.  Padded-row
    views ([..., :V] of wider rows) are taken as they are.  No host read: capturable."""
    ts = (logits, hlens, targets, ulens)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise TypeError("rnnt_loss: openeat_amd ops need CUDA tensors; there is no CPU fallback")
    if logits.dtype != torch.float32 or logits.dim() != 4:
        raise TypeError(f"rnnt_loss: logits must be a float32 (B, T, U+1, V) tensor (got {logits.dtype}, {tuple(logits.shape)})")
    B, T, U1, V = (int(s) for s in logits.shape)
    if any(t.dtype.is_floating_point or t.dtype == torch.bool for t in ts[1:]) or hlens.shape != (B,) or ulens.shape != (B,) \
            or tuple(targets.shape) != (B, U1 - 1):
        raise TypeError(f"rnnt_loss: hlens (B), targets (B, U) and ulens (B) must be integer tensors with U + 1 = {U1} "
                        f"(got {tuple(hlens.shape)}, {tuple(targets.shape)}, {tuple(ulens.shape)})")
    if not (B >= 1 and T >= 1 and U1 >= 1 and V >= 2 and 0 <= int(blank) < V):
        raise ValueError(f"rnnt_loss: B={B} T={T} U+1={U1} V={V} blank={blank}")
    pend = _PENDING_LNF.take(logits)
    if pend is not None:
        pend.resolve()
    return RNNTLossFn.apply(logits, hlens.to(torch.int32).contiguous(), targets.to(torch.int32).contiguous(),
                            ulens.to(torch.int32).contiguous(), int(blank), bool(inplace))


class JointCombineFn(torch.autograd.Function):
    """oe_joint_combine_fwd / _bwd: z[b,t,u,:] = act(e[b,t,:] + p[b,u,:]), zeros outside each utterance's lattice; the backward
    recomputes the pre-activation and sums over u (de) and over t (dp) in a fixed order."""

    @staticmethod
    def forward(ctx, e, p, hl32, ul32, act):
        e, p = _chk(e, "joint_combine"), _chk(p, "joint_combine")
        B, T, J = (int(s) for s in e.shape)
        U1 = int(p.shape[1])
        z = torch.empty(B, T, U1, J, dtype=torch.float32, device=e.device)
        a = hip.JointCombineArgs()
        a.e, a.p, a.B, a.T, a.U1, a.J, a.act = e.data_ptr(), p.data_ptr(), B, T, U1, J, int(act)
        a.hlens, a.ulens, a.z = hip.ptr(hl32), hip.ptr(ul32), z.data_ptr()
        hip.check(hip.lib().oe_joint_combine_fwd(hip.C.byref(a), hip.stream()), "oe_joint_combine_fwd")
        ctx.save_for_backward(e, p, *(t for t in (hl32, ul32) if t is not None))
        ctx.cfg = (B, T, U1, J, int(act), hl32 is not None, ul32 is not None)
        return z

    @staticmethod
    def backward(ctx, dz):
        e, p, *rest = ctx.saved_tensors
        B, T, U1, J, act, has_h, has_u = ctx.cfg
        hl32 = rest.pop(0) if has_h else None
        ul32 = rest.pop(0) if has_u else None
        dz = _chk(dz, "joint_combine gradient")
        de, dp = torch.empty_like(e), torch.empty_like(p)
        a = hip.JointCombineBwdArgs()
        a.e, a.p, a.B, a.T, a.U1, a.J, a.act = e.data_ptr(), p.data_ptr(), B, T, U1, J, act
        a.hlens, a.ulens, a.dz, a.de, a.dp = hip.ptr(hl32), hip.ptr(ul32), dz.data_ptr(), de.data_ptr(), dp.data_ptr()
        hip.check(hip.lib().oe_joint_combine_bwd(hip.C.byref(a), hip.stream()), "oe_joint_combine_bwd")
        return de, dp, None, None, None


def joint_combine(e, p, hlens=None, ulens=None, act=ACT_TANH):
    """The joint network's broadcast (oe_joint_combine_fwd): e (B, T, J) encoder side, p (B, U+1, J) predictor side ->
    z (B, T, U+1, J) = act(e[:, :, None] + p[:, None]); with hlens / ulens (B, integer, on the device) the nodes t >= hlens[b] or
    u > ulens[b] are zeros and take no gradient.  act: an ACT_* code or its name.  Differentiable in e and p."""
    if isinstance(act, str) or act is None:
        act = ACT_IDS[act or "none"]
    if not (isinstance(e, torch.Tensor) and isinstance(p, torch.Tensor) and e.dim() == 3 and p.dim() == 3 and e.shape[0] == p.shape[0]
            and e.shape[2] == p.shape[2]):
        raise TypeError("joint_combine: e (B, T, J) and p (B, U+1, J) must agree in B and J")
    B = int(e.shape[0])
    lens = []
    for name, t in (("hlens", hlens), ("ulens", ulens)):
        if t is not None:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and not t.dtype.is_floating_point and tuple(t.shape) == (B,)):
                raise TypeError(f"joint_combine: {name} must be an integer (B,) CUDA tensor")
            t = t.to(torch.int32).contiguous()
        lens.append(t)
    return JointCombineFn.apply(e, p, lens[0], lens[1], int(act))


def _prefix_score_logp(name, logp, lens, group):
    if not (isinstance(logp, torch.Tensor) and logp.is_cuda) or not (lens is None or (isinstance(lens, torch.Tensor) and lens.is_cuda)):
        raise TypeError(f"{name}: openeat_amd ops need CUDA tensors; there is no CPU fallback")
    if logp.dtype != torch.float32 or logp.dim() != 3:
        raise TypeError(f"{name}: logp must be a float32 (B, Tmax, V) tensor (got {logp.dtype}, {tuple(logp.shape)})")
    if lens is not None and (lens.dtype.is_floating_point or lens.dtype == torch.bool or lens.shape != logp.shape[:1]):
        raise TypeError(f"{name}: lens (B) must be an integer tensor")
    group = int(group)
    if group < 1:
        raise ValueError(f"{name}: group must be >= 1 (got {group})")
    return logp.contiguous(), (None if lens is None else lens.to(torch.int32).contiguous()), group


def ctc_prefix_score_init(logp, lens, group: int = 1, blank: int = 0):
    """The empty hypothesis' CTC prefix state for R = B * group rows (oe_ctc_prefix_score_init; semantics in
    include/openeat_hip.h): logp (B, Tmax, V) float32 CTC log-probabilities, lens (B) valid frames or None, on the device.
    -> state (R, Tmax, 2) float64; what lies at or behind an utterance's length is left as allocated.  Capturable."""
    logp, len32, group = _prefix_score_logp("ctc_prefix_score_init", logp, lens, group)
    B, Tmax, V = (int(s) for s in logp.shape)
    state = torch.empty(B * group, Tmax, 2, dtype=torch.float64, device=logp.device)
    hip.call("oe_ctc_prefix_score_init", logp, len32, B, Tmax, V, V, group, int(blank), state)
    return state


def ctc_prefix_score(logp, lens, state_in, hyp_len, last_tok, cand, eos: int, group: int = 1, blank: int = 0, states: bool = True,
                     cand_state=None):
    """CTC prefix scores of C candidate extensions of each of R = B * group hypotheses (oe_ctc_prefix_score; semantics in
    include/openeat_hip.h): logp (B, Tmax, V) float32, lens (B) or None, state_in (R, Tmax, 2) float64, hyp_len (R) token
    counts (< 0: the slot does not exist, its psi are -inf), last_tok (R), cand (R, C) with 1 <= C <= 64, all on the device.
    -> psi (R, C) float64 and, with `states`, cand_state (R, Tmax, C, 2) float64 - written into the tensor given as
    `cand_state` when there is one; entries of candidates that produce no state (blank, out of range, <eos>), of missing
    slots and of frames behind an utterance's length are not written.  No host read: capturable."""
    name = "ctc_prefix_score"
    logp, len32, group = _prefix_score_logp(name, logp, lens, group)
    ts = (state_in, hyp_len, last_tok, cand)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        raise TypeError(f"{name}: openeat_amd ops need CUDA tensors; there is no CPU fallback")
    B, Tmax, V = (int(s) for s in logp.shape)
    R = B * group
    if state_in.dtype != torch.float64 or tuple(state_in.shape) != (R, Tmax, 2):
        raise TypeError(f"{name}: state_in must be a float64 ({R}, {Tmax}, 2) tensor (got {state_in.dtype}, {tuple(state_in.shape)})")
    if any(t.dtype.is_floating_point or t.dtype == torch.bool for t in ts[1:]) or hyp_len.shape != (R,) or last_tok.shape != (R,) \
            or cand.dim() != 2 or cand.shape[0] != R:
        raise TypeError(f"{name}: hyp_len ({R}), last_tok ({R}) and cand ({R}, C) must be integer tensors")
    C = int(cand.shape[1])
    if not 1 <= C <= 64:
        raise ValueError(f"{name}: {C} candidates per hypothesis outside 1..64")
    dev = logp.device
    psi = torch.empty(R, C, dtype=torch.float64, device=dev)
    if states and cand_state is None:
        cand_state = torch.empty(R, Tmax, C, 2, dtype=torch.float64, device=dev)
    elif states and (cand_state.dtype != torch.float64 or tuple(cand_state.shape) != (R, Tmax, C, 2) or not cand_state.is_cuda
                     or not cand_state.is_contiguous()):
        raise TypeError(f"{name}: cand_state must be a contiguous float64 ({R}, {Tmax}, {C}, 2) CUDA tensor")
    hip.call("oe_ctc_prefix_score", logp, len32, B, Tmax, V, V, group, state_in.contiguous(), hyp_len.to(torch.int32).contiguous(),
             last_tok.to(torch.int32).contiguous(), cand.to(torch.int32).contiguous(), C, int(blank), int(eos), psi,
             cand_state if states else None)
    return (psi, cand_state) if states else psi


def topk_rows(x, k: int, log_softmax: bool = False):
    """`x.topk(k)` over the last dim - of log_softmax(x) when asked - in one kernel (asr_model.py:251, 258, 358).
    Returns (values float32, indices int64), sorted descending; ties go to the lowest index."""
    x = _chk(x, "topk_rows")
    V = x.shape[-1]
    rows = x.numel() // V
    vals = torch.empty(*x.shape[:-1], k, dtype=torch.float32, device=x.device)
    idx = torch.empty(*x.shape[:-1], k, dtype=torch.int64, device=x.device)
    hip.call("oe_topk_rows", x, rows, V, int(k), int(bool(log_softmax)), vals, idx)
    return vals, idx


def logprob_gather(logits, idx, also: int = None):
    """log_softmax(logits)[..., idx] (+ log_softmax(logits)[..., also] for one fixed column) without materialising the
    log-probabilities: logits (..., V) float32, idx (...) int64 (out-of-range entries give 0).  Returns tensors shaped like idx."""
    x = _chk(logits, "logprob_gather")
    V = x.shape[-1]
    rows = x.numel() // V
    idx = idx.to(torch.int64).contiguous()
    assert idx.numel() == rows
    out_a = torch.empty(idx.shape, dtype=torch.float32, device=x.device)
    out_b = torch.empty(idx.shape, dtype=torch.float32, device=x.device) if also is not None else None
    hip.call("oe_logprob_gather", x, rows, V, idx, 0 if also is None else int(also), out_a, out_b)
    return out_a if also is None else (out_a, out_b)


def log_softmax_rows(x):
    """log_softmax over the last dim (ctc.py:56-64, asr_model.py:484-488) on device."""
    x = _chk(x, "log_softmax")
    out = torch.empty_like(x)
    V = x.shape[-1]
    hip.call("oe_log_softmax", x, x.numel() // V, V, out)
    return out
