"""CPU: the n-gram LM.  (1) the yardstick (tests/ngram_ref.py) on a hand-worked ARPA, (2) the back-off rule itself - a built
model's probabilities sum to one in every context, (3) NgramLM.score / full_scores against the yardstick, (4) the reader's
refusals, (5) the surface (header, export, binding, alias)."""
import os
import re

import numpy as np
import pytest

import ngram_ref
from conftest import ROOT

# every value is a dyadic fraction: exact in float32, and every sum below is exact in float64
TINY = """\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.75\ta\t-0.25
-1.25\tb\t-0.125
-2.0\tc\t-1.5

\\2-grams:
-0.5\t<s> a\t-0.375
-0.625\ta b\t-0.0625
-1.5\tb </s>
-0.875\tc a

\\3-grams:
-0.25\t<s> a b
-0.3125\ta b </s>

\\end\\
"""
TINY_UNK = TINY.replace("ngram 1=5", "ngram 1=6").replace("-2.0\tc\t-1.5\n", "-2.0\tc\t-1.5\n-3.0\t<unk>\t-0.5\n")

# (model, sentence, bos, eos) -> per word (log10 p, matched order, oov), n, S
HAND = [
    # hits: <s> a (2), <s> a b at the top order, a b </s> at the top order
    ("tiny", "a b", True, True, [(-0.5, 2, False), (-0.25, 3, False), (-0.3125, 3, False)], 3, 1.0625),
    # c | <s> a: backoff(<s> a) + backoff(a) + p(c): two levels;  </s> | a c: context (a c) unlisted -> 0, backoff(c) + p(</s>)
    ("tiny", "a c", True, True, [(-0.5, 2, False), (-0.375 - 0.25 - 2.0, 1, False), (-1.5 - 1.0, 1, False)], 6, 5.625),
    # b | <s>: backoff(<s>) + p(b);  </s> | <s> b: (<s> b) unlisted -> 0, then b </s> is listed
    ("tiny", "b", True, True, [(-0.5 - 1.25, 1, False), (-1.5, 2, False)], 3, 3.25),
    # out of vocabulary, no <unk> in the file: -100, back-off 0 (a listed value: it counts as a term)
    ("tiny", "x", True, True, [(-0.5 - 100.0, 1, True), (0.0 - 1.0, 1, False)], 4, 101.5),
    # out of vocabulary, the file's own <unk>
    ("unk", "x", True, True, [(-0.5 - 3.0, 1, True), (-0.5 - 1.0, 1, False)], 4, 5.0),
    # the empty sentence: </s> | <s>
    ("tiny", "", True, True, [(-0.5 - 1.0, 1, False)], 2, 1.5),
    ("tiny", "", True, False, [], 0, 0.0),
    ("tiny", "", False, False, [], 0, 0.0),
    # bos / eos off
    ("tiny", "a b", False, False, [(-0.75, 1, False), (-0.625, 2, False)], 2, 1.375),
    ("tiny", "a b", False, True, [(-0.75, 1, False), (-0.625, 2, False), (-0.3125, 3, False)], 3, 1.6875),
    ("tiny", "a b", True, False, [(-0.5, 2, False), (-0.25, 3, False)], 2, 0.75),
    # c a b: c | <s> backs off, c a is listed (no back-off written: 0), c a b is not: backoff(c a) = 0 + a b
    ("tiny", "c a b", True, True, [(-0.5 - 2.0, 1, False), (-0.875, 2, False), (0.0 - 0.625, 2, False), (-0.3125, 3, False)], 6, 4.3125),
]


@pytest.fixture()
def tiny(tmp_path):
    paths = {}
    for name, text in (("tiny", TINY), ("unk", TINY_UNK)):
        paths[name] = str(tmp_path / f"{name}.arpa")
        open(paths[name], "w").write(text)
    return paths


def test_yardstick_on_a_hand_worked_arpa(tiny):
    lms = {k: ngram_ref.RefLM(p) for k, p in tiny.items()}
    assert lms["tiny"].order == 3
    for name, sent, bos, eos, want, n, S in HAND:
        got, gn, gS = lms[name].full_scores(sent, bos, eos)
        assert got == want, (name, sent, bos, eos, got)
        assert (gn, gS) == (n, S), (name, sent, bos, eos, gn, gS)
        assert lms[name].score(sent, bos, eos)[0] == sum(v for v, _, _ in want)


def test_product_on_the_hand_worked_arpa(tiny):
    from openeat_amd.models.ngram_lm import NgramLM
    t2c = ["a", "b", "c", "x"]
    lms = {k: NgramLM(p, t2c) for k, p in tiny.items()}
    for name, sent, bos, eos, want, _, _ in HAND:
        assert lms[name].full_scores(sent, bos, eos) == want, (name, sent, bos, eos)
        assert lms[name].score(sent, bos, eos) == sum(v for v, _, _ in want)
    lm = lms["tiny"]
    assert lm.tok2word.tolist() == [lm.word_id["a"], lm.word_id["b"], lm.word_id["c"], lm.unk_word]
    assert not isinstance(lm, __import__("torch").nn.Module)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_built_model_sums_to_one_in_every_context(tmp_path, order):
    """The back-off rule, not an implementation against a copy of itself: on a normalised model sum_w 10**p(w | h) = 1 over
    all words but <s>, for every listed context and for unlisted ones.  1e-5: a float32 log10 value of magnitude up to 5
    carries a relative error of at most 5 * 2**-24 * ln 10 = 7e-7 into its probability, and the probabilities sum to one."""
    rng = np.random.default_rng(5)
    vocab = [f"t{i}" for i in range(40)]
    # a skewed corpus (so that many n-grams repeat and many never occur)
    pw = 1.0 / np.arange(1, 41)
    pw /= pw.sum()
    corpus = [[vocab[i] for i in rng.choice(40, size=rng.integers(1, 12), p=pw)] for _ in range(600)]
    path = str(tmp_path / "built.arpa")
    ngram_ref.build_arpa(path, corpus, order, vocab, with_unk=(order % 2 == 1))
    lm = ngram_ref.RefLM(path)
    assert lm.order == order
    words = [w for w in lm.words if w != "<s>"]
    contexts = [g for g in lm.grams if len(g) < order and g[-1] != "</s>" and "<s>" not in g[1:]] + [()]
    for _ in range(50):                                    # unlisted ones (checked to be so)
        h = tuple(vocab[i] for i in rng.integers(0, 40, max(order - 1, 1)))[: order - 1]
        if h not in lm.grams:
            contexts.append(h)
    worst = 0.0
    for h in contexts:
        total = sum(10.0 ** lm.p(w, h)[0] for w in words)
        worst = max(worst, abs(total - 1.0))
    print(f"order {order}: {len(lm.grams)} n-grams, {len(contexts)} contexts, worst |sum - 1| = {worst:.3g}")
    assert worst <= 1e-5


def _random_sentences(rng, words, count, max_len=12):
    out = []
    for _ in range(count):
        n = int(rng.integers(0, max_len + 1))
        sent = [words[i] for i in rng.integers(0, len(words), n)]
        for j in range(n):
            if rng.random() < 0.1:
                sent[j] = "zz" + str(int(rng.integers(0, 3)))          # out of vocabulary
        out.append((" ".join(sent), bool(rng.random() < 0.8), bool(rng.random() < 0.8)))
    return out


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_product_equals_yardstick_on_random_sentences(tmp_path, order):
    """NgramLM.score / full_scores == the yardstick: orders and oov flags exactly, values within 2**-52 * n * S (both sum the
    same float32 values in float64; only the order of the additions may differ)."""
    from openeat_amd.models.ngram_lm import NgramLM
    rng = np.random.default_rng(100 + order)
    for with_unk in (True, False):
        path = str(tmp_path / f"r{order}{int(with_unk)}.arpa")
        words = ngram_ref.random_arpa(path, order, 12, 300, rng, with_unk=with_unk)
        ref = ngram_ref.RefLM(path)
        lm = NgramLM(path, {i: w for i, w in enumerate(words)})
        assert lm.order == order
        assert lm.capacity >= 2 * (len(ref.grams) - len(ref.words)) and lm.capacity & (lm.capacity - 1) == 0
        for sent, bos, eos in _random_sentences(rng, words, 100):
            want, n, S = ref.full_scores(sent, bos, eos)
            got = lm.full_scores(sent, bos, eos)
            tol = 2.0 ** -52 * n * S
            assert [(o, v) for _, o, v in got] == [(o, v) for _, o, v in want], (sent, bos, eos)
            assert all(abs(a[0] - b[0]) <= tol for a, b in zip(got, want)), (sent, bos, eos)
            assert abs(lm.score(sent, bos, eos) - ref.score(sent, bos, eos)[0]) <= tol, (sent, bos, eos)


def test_product_equals_yardstick_on_a_built_model(tmp_path):
    from openeat_amd.models.ngram_lm import NgramLM
    rng = np.random.default_rng(9)
    vocab = [str(i) for i in range(30)]
    corpus = [[vocab[i] for i in rng.integers(0, 30, rng.integers(1, 10))] for _ in range(400)]
    path = str(tmp_path / "built.arpa")
    ngram_ref.build_arpa(path, corpus, 3, vocab)
    ref, lm = ngram_ref.RefLM(path), NgramLM(path, {i: w for i, w in enumerate(vocab)})
    for sent, bos, eos in _random_sentences(rng, vocab, 200):
        want, n, S = ref.full_scores(sent, bos, eos)
        got = lm.full_scores(sent, bos, eos)
        assert [(o, v) for _, o, v in got] == [(o, v) for _, o, v in want]
        assert all(abs(a[0] - b[0]) <= 2.0 ** -52 * n * S for a, b in zip(got, want))


def test_reader_errors_carry_the_line_number(tmp_path):
    from openeat_amd.models.ngram_lm import NgramLM

    def load(text, t2c=("a", "b", "c")):
        p = str(tmp_path / "bad.arpa")
        open(p, "w").write(text)
        return NgramLM(p, list(t2c))

    load(TINY)                                             # the unchanged file is fine
    with pytest.raises(ValueError, match=r":13:"):         # wrong count: the 1-gram section closes at line 13 with 5, not 6
        load(TINY.replace("ngram 1=5", "ngram 1=6"))
    orphan = TINY.replace("-0.5\t<s> a\t-0.375\n", "").replace("ngram 2=4", "ngram 2=3")    # <s> a b without <s> a
    at = orphan.split("\n").index("-0.25\t<s> a b") + 1
    with pytest.raises(ValueError, match=rf":{at}:.*context"):
        load(orphan)
    with pytest.raises(ValueError, match=r"missing \\end\\"):
        load(TINY.replace("\\end\\\n", ""))
    high = TINY.replace("ngram 3=2\n", "ngram 3=2\nngram 4=0\nngram 5=0\nngram 6=1\n")
    with pytest.raises(ValueError, match=r":7:.*order 6"):
        load(high)
    with pytest.raises(ValueError, match="whitespace"):
        load(TINY, t2c=("a", "b c"))
    with pytest.raises(ValueError, match="not in the 1-gram section"):
        load(TINY.replace("-0.875\tc a", "-0.875\tc q"))


def test_surface_header_export_binding_alias():
    import ctypes
    from openeat_amd import hip, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "openeat_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+oe_ngram_score\s*\(", src)
    assert "oe_ngram_score" in hip.exported_symbols()
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "openeat_amd", "lib", "libopeneat_hip.so")), "oe_ngram_score")
    from openeat.models.ngram_lm import NgramLM
    from openeat_amd.models.ngram_lm import NgramLM as Own
    assert NgramLM is Own and callable(ops.ngram_score)
    # arguments are checked before anything is launched
    for model in (None, hip.NgramModel(None, None, None, 2, 1, 0, 3, 0, 0, 0, 1)):         # no model; one whose pointers are NULL
        rc = hip.lib().oe_ngram_score(model, None, 0, None, 1, 1, 1, None, None, None, None)
        assert rc != 0 and b"null" in hip.lib().oe_last_error()


def test_ngram_score_has_no_cpu_fallback(tiny):
    import torch
    from openeat_amd import ops
    from openeat_amd.models.ngram_lm import NgramLM
    lm = NgramLM(tiny["tiny"], ["a", "b", "c"])
    with pytest.raises(TypeError):
        ops.ngram_score(lm, torch.zeros(2, 3, dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32))
