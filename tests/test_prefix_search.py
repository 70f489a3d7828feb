"""CPU: hip.PrefixSearch, the description of one device CTC prefix beam search (no kernel launched; NgramLM and ContextGraph
build on the host): the first-pass rule of attention_rescoring_batch as a truth table, every refusal of validate, equality /
hash / lifetime of a spec as a dict key, and the output plan of the four variants."""
import gc
import itertools
import weakref

import numpy as np
import pytest
import torch

import ngram_ref
from openeat_amd import hip
from openeat_amd.hip import PrefixSearch
from openeat_amd.models.ngram_lm import NgramLM
from openeat_amd.utils.context_graph import ContextGraph


@pytest.fixture
def arpa(tmp_path):
    path = str(tmp_path / "s.arpa")
    words = ngram_ref.random_arpa(path, 2, 10, 30, np.random.default_rng(1))
    return path, ["<blank>"] + words


def _graph():
    return ContextGraph([(1, 2), (2, 3, 4)], 0.37)


def test_first_pass_truth_table(arpa):
    ngram, module, graph = NgramLM(*arpa), torch.nn.Identity(), _graph()
    beam, bonus = 4, 0.4
    n = 0
    for lm, flag, lm_weight, fp_weight, context in itertools.product((None, ngram, module), (False, True), (0, 3.0), (None, 0.7),
                                                                     (None, graph)):
        spec = PrefixSearch.first_pass(beam, lm, lm_weight, flag, fp_weight, bonus, context)
        where = (type(lm).__name__, flag, lm_weight, fp_weight, context is not None)
        enters = flag and lm is ngram and lm_weight > 0
        if enters:
            want = (beam, ngram, context, 0.7 if fp_weight is not None else 3.0, bonus, True, True)
        elif context is not None:
            want = (beam, None, graph, 0.0, bonus, True, True)
        else:
            want = (beam, None, None, 0.0, 0.0, True, True)
        got = (spec.beam, spec.lm, spec.context, spec.lm_weight, spec.length_bonus, spec.eos, spec.final)
        assert all(g is w if i in (1, 2) else (g == w and type(g) is type(w)) for i, (g, w) in enumerate(zip(got, want))), (where, got)
        assert spec.plain == (not enters and context is None), where
        n += 1
    assert n == 48


def test_validate_refuses_and_passes(arpa):
    lm, graph = NgramLM(*arpa), _graph()
    for spec in (PrefixSearch(4), PrefixSearch(1, lm), PrefixSearch(16, None, graph), PrefixSearch(4, lm, graph, 0.7, 0.4, False, False)):
        assert spec.validate("caller", True) is None
    bad = [(PrefixSearch(4, torch.nn.Identity()), True, ()), (PrefixSearch(4, graph), True, ()), (PrefixSearch(4, None, lm), True, ()),
           (PrefixSearch(4, lm, "hotword"), True, ()), (PrefixSearch(0, lm), True, ()), (PrefixSearch(17, None, graph), True, ()),
           (PrefixSearch(17), True, ()), (PrefixSearch(4, lm, graph), False, ()), (PrefixSearch(4), False, ()),
           (PrefixSearch(4), True, ("lm",)), (PrefixSearch(4, lm), True, ("context",))]
    for spec, device_beam, require in bad:
        with pytest.raises(ValueError, match="the_caller"):
            spec.validate("the_caller", device_beam, require)
    assert PrefixSearch(4, lm, graph).validate("caller", True, ("lm", "context")) is None


def test_a_spec_is_a_key_that_keeps_its_lm_alive(arpa):
    lm, graph = NgramLM(*arpa), _graph()
    a, b = PrefixSearch(4, lm, graph, 0.7, 0.4), PrefixSearch(4, lm, graph, 0.7, 0.4)
    assert a is not b and a == b and hash(a) == hash(b) and len({a, b}) == 1
    twin = NgramLM(*arpa)                                                   # the same model, another object: another search
    assert PrefixSearch(4, twin, graph, 0.7, 0.4) != a and PrefixSearch(4, lm, _graph(), 0.7, 0.4) != a
    for other in (PrefixSearch(5, lm, graph, 0.7, 0.4), PrefixSearch(4, lm, graph, 0.5, 0.4), PrefixSearch(4, lm, graph, 0.7, 0.0),
                  PrefixSearch(4, lm, graph, 0.7, 0.4, False), PrefixSearch(4, lm, graph, 0.7, 0.4, True, False), PrefixSearch(4, lm, None, 0.7, 0.4)):
        assert other != a
    with pytest.raises(Exception):
        a.beam = 5                                                          # frozen
    cache = {("s1", (5, 97, 80), a): "capture"}
    alive = weakref.ref(lm)
    del lm, a, b, other
    gc.collect()
    assert alive() is not None and cache[("s1", (5, 97, 80), PrefixSearch(4, alive(), graph, 0.7, 0.4))] == "capture"
    cache.clear()
    gc.collect()
    assert alive() is None


def test_the_output_plan_of_the_four_variants(arpa):
    lm, graph = NgramLM(*arpa), _graph()
    buf = {k: torch.full((2, 4), float(i), dtype=torch.float64) for i, k in enumerate(hip.SCORES)}
    total, ctc, lms, bias = (buf[k] for k in hip.SCORES)
    assert hip.SCORES == ("total", "ctc", "lm", "bias")
    # (the plan; what the kernel is handed as out_score, out_ctc, out_lm, out_bias; what the caller sees of four buffers)
    table = [(PrefixSearch(4), dict(total=True), [total, None, None, None], dict(total=total, ctc=total, lm=lms, bias=bias)),
             (PrefixSearch(4, lm), dict(total=True, ctc=True, lm=True), [total, ctc, lms, None], dict(total=total, ctc=ctc, lm=lms, bias=bias)),
             (PrefixSearch(4, None, graph), dict(total=True, ctc=True, lm=False, bias=True), [total, ctc, None, bias],
              dict(total=total, ctc=ctc, lm=lms, bias=bias)),
             (PrefixSearch(4, lm, graph), dict(total=True, ctc=True, lm=True, bias=True), [total, ctc, lms, bias],
              dict(total=total, ctc=ctc, lm=lms, bias=bias))]
    for spec, plan, outs, seen in table:
        assert spec.plan == plan and list(spec.plan) == list(plan)
        got_outs, got_seen = spec.bind(buf)
        assert len(got_outs) == 4 and all(g is w for g, w in zip(got_outs, outs))
        assert list(got_seen) == list(hip.SCORES) and all(got_seen[k] is seen[k] for k in hip.SCORES)
        # a one-shot search holds the plan's buffers only: the caller sees None for the others, and ctc is still the total
        own = {k: buf[k] for k in plan}
        got_outs, got_seen = spec.bind(own)
        assert all(g is w for g, w in zip(got_outs, outs))
        assert all(got_seen[k] is (seen[k] if k in plan or (k == "ctc" and spec.plain) else None) for k in hip.SCORES)
