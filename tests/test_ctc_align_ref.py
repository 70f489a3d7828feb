"""CPU: the float64 alignment helper against brute force, and the host-side surface of CTC forced alignment (header, binding,
signatures, frame times).  No compute is launched here."""
import inspect
import itertools
import os
import re

import numpy as np

import ctc_align_ref as R
from conftest import ROOT


def brute_force(lp, y):
    """Best log-probability over EVERY length-T frame path that collapses to y."""
    T, V = lp.shape
    best = -np.inf
    for path in itertools.product(range(V), repeat=T):
        if R.collapse(path) == list(y):
            best = max(best, sum(lp[t, c] for t, c in enumerate(path)))
    return best


def test_helper_equals_brute_force_enumeration():
    rng = np.random.default_rng(0)
    V, feasible, infeasible = 4, 0, 0
    for case in range(60):
        T = int(rng.integers(1, 7))
        L = int(rng.integers(0, 4))
        y = [int(c) for c in rng.integers(1, V, size=L)]
        if L >= 2 and case % 3 == 0:
            y[1] = y[0]                                   # an adjacent repeat needs a blank between
        lp = R.log_softmax(rng.standard_normal((T, V)) * 2)
        want = brute_force(lp, y)
        score, states, tokens = R.align(lp, y)
        need = L + sum(1 for i in range(1, L) if y[i] == y[i - 1])
        if T < need:
            infeasible += 1
            assert want == -np.inf and score == -np.inf and states is None and tokens is None
            continue
        feasible += 1
        assert abs(score - want) <= 1e-12, (case, score, want)
        assert R.collapse(tokens) == y and len(tokens) == T
        ext = R.ext_labels(y)
        assert abs(R.path_score(lp, ext, states) - score) <= 1e-12
        assert states[0] in (0, 1) and states[-1] in (2 * L, 2 * L - 1)
        assert all(R.legal_move(ext, a, b) for a, b in zip(states, states[1:]))
    assert feasible >= 30 and infeasible >= 5, (feasible, infeasible)


def test_helper_tie_rule():
    # all log-probs equal: every legal path ties.  Stay wins wherever the state was reachable a frame earlier, so seen from
    # the end the path sits in its last state as long as it can: 4 is first reachable at t = 2 (1 -> skip -> 3 -> 4)
    lp = np.full((5, 3), -1.0)
    score, states, tokens = R.align(lp, [1, 2])
    assert score == -5.0
    assert states == [1, 3, 4, 4, 4] and tokens == [1, 2, 0, 0, 0]
    assert R.spans(states, 2) == ([0, 1], [0, 1])
    assert R.align(np.full((0, 3), -1.0), [1])[0] == -np.inf
    assert R.align(np.full((2, 3), -1.0), [1, 1])[0] == -np.inf          # a repeat needs three frames
    assert R.align(np.full((3, 3), -1.0), [])[2] == [0, 0, 0]            # empty target: all blank


def test_header_declares_and_binding_holds_the_aligner():
    from openeat_amd import hip
    src = open(os.path.join(ROOT, "include", "openeat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("oe_ctc_align", "oe_ctc_align_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src), name + " not declared in include/openeat_hip.h"
        assert name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)


def test_bad_arguments_are_reported_not_launched():
    from openeat_amd import hip
    lib = hip.lib()
    assert lib.oe_ctc_align(None, 8, 1, 4, 8, None, None, 2, None, None, None, None, None, None, None, None) != 0
    assert b"oe_ctc_align: null pointer" in lib.oe_last_error()
    assert lib.oe_ctc_align_workspace_bytes(2, 10, 3) >= 2 * 10 * 7 * 4


def test_python_surface():
    from openeat_amd.models.asr_model import ASRModel
    from openeat_amd.modules.ctc import CTC
    from openeat_amd import ops
    import openeat.models.asr_model
    assert list(inspect.signature(CTC.forced_align).parameters) == ["self", "hs_pad", "hlens", "ys_pad", "ys_lens"]
    p = list(inspect.signature(ASRModel.ctc_align).parameters)
    assert p[:5] == ["self", "features", "features_length", "targets", "targets_length"] and "with_times" in p
    assert list(inspect.signature(ops.ctc_align).parameters) == ["logits", "ldv", "B", "T", "V", "hlens", "ys", "ylens"]
    assert openeat.models.asr_model.ASRModel.ctc_align is ASRModel.ctc_align


def test_frame_times():
    from openeat_amd.utils.align import frame_times
    import openeat.utils.align
    assert openeat.utils.align.frame_times is frame_times
    assert frame_times(0, 0, 4) == (0.0, 0.04)
    assert frame_times(25, 49, 4) == (1.0, 2.0)
    assert frame_times(3, 5, 6, frame_shift_ms=12.5) == (0.225, 0.45)
    assert frame_times(10, 10, 1) == (0.1, 0.11)
