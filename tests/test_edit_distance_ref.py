"""CPU: the edit-distance yardstick (edit_distance_ref.py) against what the reference's error-rate tool answered
(golden/f26_edit_distance.json, written by golden/make_edit_distance_fixture.py), hand-worked pairs where the tie order decides
the counts, the error-rate bookkeeping, and the host-side surface of oe_edit_distance.  No compute is launched here."""
import ctypes
import math
import os
import re

import torch

import edit_distance_ref as R
from conftest import ROOT, load_golden_json


def test_yardstick_equals_the_reference_tool_on_every_golden_record():
    records = load_golden_json("f26_edit_distance")
    assert len(records) == 288
    assert {r["vocab"] for r in records} == {2, 3, 5, 50}
    assert {(len(r["ref"]), len(r["hyp"])) for r in records} == {(n, m) for n in (0, 1, 2, 5, 17, 40) for m in (0, 1, 2, 5, 17, 40)}
    ties = 0
    for rec in records:
        (cor, sub, dele, ins), r2h = R.edit_distance(rec["ref"], rec["hyp"])
        assert (cor + sub + dele, cor, sub, dele, ins) == (rec["all"], rec["cor"], rec["sub"], rec["del"], rec["ins"]), rec
        assert rec["all"] == len(rec["ref"]) and cor + sub + ins == len(rec["hyp"])
        # the alignment is the counts' own: matched positions ascend, equal tokens are cor, the rest of the reference is deleted
        pos = [j for j in r2h if j >= 0]
        assert pos == sorted(set(pos)) and len(pos) == cor + sub and r2h.count(-1) == dele
        assert sum(rec["ref"][i] == rec["hyp"][j] for i, j in enumerate(r2h) if j >= 0) == cor
        ties += (sub + dele + ins) > 0 and rec["vocab"] <= 3
    assert ties > 50


def test_tie_order_decides_the_counts():
    a, b = 7, 9
    # r = a b, h = b a.  D = [[0 1 2] [1 1 1] [2 1 2]].  At (2, 2) deletion (1, 2) + 1 = 2 comes first; insertion (2, 1) + 1 = 2 and
    # the substitution (1, 1) + 1 = 2 are not strictly smaller.  (1, 2) is the match a = a from (0, 1), which is an insertion:
    #   ref:  -  a  b
    #   hyp:  b  a  -        one cor, one del, one ins - not the two substitutions of the same cost
    assert R.edit_distance([a, b], [b, a]) == ((1, 0, 1, 1), [1, -1])
    # r = a, h = b b.  At (1, 2): deletion 3, insertion (1, 1) + 1 = 2 wins, the substitution (0, 1) + 1 = 2 is not strictly smaller:
    # a is substituted by the FIRST b, the second is inserted
    assert R.edit_distance([a], [b, b]) == ((0, 1, 0, 1), [0])
    # r = a a, h = a.  At (2, 1): deletion (1, 1) + 1 = 1 first, the match (1, 0) + 0 = 1 is not strictly smaller: the FIRST a matches
    assert R.edit_distance([a, a], [a]) == ((1, 0, 1, 0), [0, -1])
    # r = a, h = a a.  At (1, 2): insertion (1, 1) + 1 = 1 beats deletion 3, the match (0, 1) + 0 = 1 is not strictly smaller
    assert R.edit_distance([a], [a, a]) == ((1, 0, 0, 1), [0])
    # r = a b a, h = b.  (3, 1): deletion (2, 1) + 1 = 2 first; (2, 1) is the match b = b from (1, 0)
    assert R.edit_distance([a, b, a], [b]) == ((1, 0, 2, 0), [-1, 0, -1])
    assert R.edit_distance([], []) == ((0, 0, 0, 0), [])
    assert R.edit_distance([a, b], []) == ((0, 0, 2, 0), [-1, -1])
    assert R.edit_distance([], [a, b, a]) == ((0, 0, 0, 3), [])


def test_error_rate_overall_line_and_result():
    from openeat_amd.utils.error_rate import ErrorRate, nbest_oracle, overall_line
    er = ErrorRate()
    assert er.result()["all"] == 0 and math.isnan(er.result()["rate"])
    assert str(er) == "Overall -> 0.00 % N=0 C=0 S=0 D=0 I=0"
    er.update(torch.tensor([[98000, 6000, 100, 200], [-1, -1, -1, -1]], dtype=torch.int32))
    er.update(torch.tensor([[470, 150, 45, 21]], dtype=torch.int32))
    assert str(er) == "Overall -> 6.22 % N=104765 C=98470 S=6150 D=145 I=221"
    res = er.result()
    assert res == {"all": 104765, "cor": 98470, "sub": 6150, "del": 145, "ins": 221, "rate": (6150 + 145 + 221) / 104765}
    assert overall_line(res) == str(er)
    one = ErrorRate().update(torch.tensor([[0, 1, 2, 9]]))
    assert str(one) == "Overall -> 400.00 % N=3 C=0 S=1 D=2 I=9"
    # oracle: fewest errors among the slots that exist, the lowest index among equals
    c = torch.tensor([[5, 1, 0, 1], [4, 1, 1, 0], [6, 0, 0, 0], [-1, -1, -1, -1],
                      [-1, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1], [0, 3, 0, 0],
                      [2, 1, 0, 0], [1, 0, 2, 0], [3, 0, 0, 1], [1, 1, 1, 0]], dtype=torch.int32)
    best, index = nbest_oracle(c, 4)
    assert index.tolist() == [2, 3, 0] and best.tolist() == [[6, 0, 0, 0], [0, 3, 0, 0], [2, 1, 0, 0]]
    import openeat.utils.error_rate as alias
    assert alias.ErrorRate is ErrorRate


def test_header_declares_and_binding_holds_edit_distance():
    from openeat_amd import hip
    src = open(os.path.join(ROOT, "include", "openeat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("oe_edit_distance", "oe_edit_distance_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src), name + " not declared in include/openeat_hip.h"
        assert name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)


def test_bad_arguments_are_reported_not_launched():
    from openeat_amd import hip
    lib = hip.lib()
    host = (ctypes.c_int * 8)()                     # stands in for every pointer: a rejected call dereferences nothing
    p = ctypes.cast(host, ctypes.c_void_p)

    def call(ref_ld=8, group=1, hyp_ld=8, P=4, Nmax=8, Mmax=8, counts=p, lens=p):
        return lib.oe_edit_distance(p, ref_ld, lens, group, p, hyp_ld, lens, P, Nmax, Mmax, counts, None, None, None)

    for kwargs, say in ((dict(Nmax=1024, ref_ld=1024), b"1023-token limit"), (dict(Mmax=1024, hyp_ld=1024), b"1023-token limit"),
                        (dict(group=0), b"group must be >= 1"), (dict(P=4, group=3), b"not a multiple of group"),
                        (dict(ref_ld=7), b"leading dimensions"), (dict(hyp_ld=7), b"leading dimensions"),
                        (dict(counts=None), b"null pointer"), (dict(lens=None), b"null pointer"), (dict(Nmax=-1), b"bad shape")):
        assert call(**kwargs) != 0, kwargs
        assert say in lib.oe_last_error(), (kwargs, lib.oe_last_error())
    # an aligned call whose back-pointers do not fit LDS needs its workspace
    assert lib.oe_edit_distance(p, 1023, p, 1, p, 1023, p, 1, 1023, 1023, p, p, None, None) != 0
    assert b"null workspace" in lib.oe_last_error()
    W = 64                                          # words of 16 two-bit moves per row at Mmax = 1023
    assert lib.oe_edit_distance_workspace_bytes(5, 1023, 1023) == 5 * 1023 * W * 4
    assert lib.oe_edit_distance_workspace_bytes(144, 257, 257) == 0          # 257 * 17 words: in LDS
    assert lib.oe_edit_distance_workspace_bytes(0, 1023, 1023) == 0


def test_python_surface():
    import inspect
    from openeat_amd import ops
    from openeat_amd.models.asr_model import ASRModel
    assert list(inspect.signature(ops.edit_distance).parameters) == ["ref", "ref_lens", "hyp", "hyp_lens", "group", "align"]
    sig = inspect.signature(ASRModel.error_counts).parameters
    assert list(sig)[:8] == ["self", "features", "features_length", "targets", "targets_length", "mode", "beam_size", "nbest_oracle"]
    assert sig["mode"].default == "ctc_greedy_search" and sig["beam_size"].default == 10 and sig["nbest_oracle"].default is False
    z = torch.zeros(2, 3, dtype=torch.int64)
    try:
        ops.edit_distance(z, torch.zeros(2, dtype=torch.int64), z, torch.zeros(2, dtype=torch.int64))
    except TypeError as e:
        assert "CUDA tensors" in str(e)
    else:
        raise AssertionError("CPU tensors must raise")


def test_executor_cv_error_rate_bookkeeping_with_a_stub_model():
    """Executor.cv's part alone (the model here is a stub that hands out fixed counts; the real one runs in the GPU file)."""
    from openeat_amd.utils.executor import Executor

    class Stub(torch.nn.Module):
        def forward(self, x):
            return x.sum() * 0 + 1.5, torch.tensor(0.25)

        def error_counts(self, x):
            return {"counts": torch.tensor([[3, 1, 0, 2], [-1, -1, -1, -1], [4, 0, 1, 0]], dtype=torch.int32)}

    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    loader = [(["a", "b", "c"], {"x": torch.ones(3)}), ([], {"x": torch.ones(3)}), (["d", "e", "f"], {"x": torch.ones(3)})]
    runs = {}
    for name, args in (("absent", {"log_interval": 1}), ("false", {"log_interval": 1, "cv_error_rate": False}),
                       ("on", {"log_interval": 1, "cv_error_rate": True})):
        ex, log = Executor(), Log()
        runs[name] = (ex, log.lines, ex.cv(log, Stub(), loader, "cpu", args))
    ex, lines, pair = runs["on"]
    assert pair == (1.5, 0.25)
    assert ex.last_cv_error_rate == {"all": 18, "cor": 14, "sub": 2, "del": 2, "ins": 4, "rate": 8 / 18}      # the empty batch is skipped
    assert lines[-1] == "CV TER Overall -> 44.44 % N=18 C=14 S=2 D=2 I=4" and sum(l.startswith("CV TER") for l in lines) == 1
    for name in ("absent", "false"):
        ex_off, lines_off, pair_off = runs[name]
        assert not hasattr(ex_off, "last_cv_error_rate") and lines_off == lines[:-1] and pair_off == pair
