"""The yardstick for the n-gram LM tests: the ARPA back-off definition written down as directly as possible, independent of
openeat_amd (a dict of word tuples and a recursion in float64; no tables, no hashing, no ids).

    p(w | h) = logp(h w)                        if the n-gram `h w` is listed
             = backoff(h) + p(w | h[1:])        otherwise, with backoff(h) = 0 when h is not listed

h = the last order-1 words, starting from <s> when bos (context only, never scored), </s> scored when eos; a word that is
not a listed unigram is <unk>, which has log10 p = -100 and back-off 0 when the file does not list it.  Values are rounded
to float32 on load (np.float32(float(text))) and summed in float64.

Also here: a count-based builder of a NORMALISED ARPA (interpolated absolute discounting) and a generator of RANDOM ARPAs
(arbitrary values, random n-gram sets closed under "the first k-1 words of a listed k-gram are listed") for lookup stress."""
import numpy as np

UNK_LOGP = np.float32(-100.0)


def read_arpa(path):
    """-> (order, {tuple of words: (float32 log10 p, float32 back-off)})."""
    grams, order, k = {}, 0, 0
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\"):
                k = int(line[1:line.index("-")])
                order = max(order, k)
                continue
            fields = line.split()
            bo = np.float32(float(fields[k + 1])) if len(fields) > k + 1 else np.float32(0.0)
            grams[tuple(fields[1:k + 1])] = (np.float32(float(fields[0])), bo)
    return order, grams


class RefLM:
    def __init__(self, path):
        self.order, self.grams = read_arpa(path)
        if ("<unk>",) not in self.grams:
            self.grams[("<unk>",)] = (UNK_LOGP, np.float32(0.0))
        self.words = [g[0] for g in self.grams if len(g) == 1]

    def p(self, w, h):
        """log10 p(w | h) for a word w that is a listed unigram -> (value, matched order, [the float32 values summed])."""
        g = tuple(h) + (w,)
        if g in self.grams:
            v = self.grams[g][0]
            return float(v), len(g), [float(v)]
        assert len(h) > 0, f"{w!r} is not a listed unigram"
        v, o, terms = self.p(w, tuple(h)[1:])
        if tuple(h) in self.grams:
            b = float(self.grams[tuple(h)][1])
            return b + v, o, [b] + terms
        return v, o, terms

    def full_scores(self, sentence, bos=True, eos=True):
        """-> ([(log10 p, matched order, oov) per word, and for </s> when eos], n, S): n float32 values were summed in all,
        S = the sum of their magnitudes."""
        words = sentence.split()
        oov = [(w,) not in self.grams for w in words]
        seq = (["<s>"] if bos else []) + [w if (w,) in self.grams else "<unk>" for w in words] + (["</s>"] if eos else [])
        off = 1 if bos else 0
        out, n, S = [], 0, 0.0
        for i in range(off, len(seq)):
            h = tuple(seq[max(0, i - (self.order - 1)):i])
            v, o, terms = self.p(seq[i], h)
            out.append((v, o, oov[i - off] if i - off < len(words) else False))
            n += len(terms)
            S += sum(abs(t) for t in terms)
        return out, n, S

    def score(self, sentence, bos=True, eos=True):
        out, n, S = self.full_scores(sentence, bos, eos)
        return sum(v for v, _, _ in out), n, S


def _fmt(v):
    return f"{float(np.float32(v)):.9g}"


def write_arpa(path, by_order):
    """by_order[k-1] = [(words tuple, log10 p, back-off or None)]."""
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k, rows in enumerate(by_order, 1):
            f.write(f"ngram {k}={len(rows)}\n")
        for k, rows in enumerate(by_order, 1):
            f.write(f"\n\\{k}-grams:\n")
            for words, lp, bo in rows:
                f.write(_fmt(lp) + "\t" + " ".join(words) + ("" if bo is None else "\t" + _fmt(bo)) + "\n")
        f.write("\n\\end\\\n")


def build_arpa(path, corpus, order, vocab, discount=0.5, with_unk=True):
    """A normalised ARPA of `order` from `corpus` (lists of words out of `vocab`): interpolated absolute discounting,
        p_k(w | h) = max(c(h w) - D, 0) / c(h .) + D N1+(h .) / c(h .) * p_{k-1}(w | h[1:]),   p_1(w) = (c(w) + 1) / (N + |W|)
    over W = vocab + </s> (+ <unk>); the listed k-grams are the seen ones, backoff(h) = log10(D N1+(h .) / c(h .)) - which is
    exactly the ARPA back-off rule for an unseen w, so every context's probabilities sum to one.  <s> has log10 p = -99."""
    import math
    from collections import Counter, defaultdict
    W = list(vocab) + ["</s>"] + (["<unk>"] if with_unk else [])
    counts = [Counter() for _ in range(order)]
    for sent in corpus:
        seq = ["<s>"] + list(sent) + ["</s>"]
        for k in range(1, order + 1):
            for i in range(len(seq) - k + 1):
                counts[k - 1][tuple(seq[i:i + k])] += 1
    N = sum(c for g, c in counts[0].items() if g != ("<s>",))
    prob = [{(w,): (counts[0][(w,)] + 1) / (N + len(W)) for w in W}]
    gamma = [{}]

    def p_of(k, g):                                        # p_k(g[-1] | g[:-1]), g of length k, by the model's own rule
        if k == 1:
            return prob[0][g]
        if g in prob[k - 1]:
            return prob[k - 1][g]
        h = g[:-1]
        return gamma[k - 1].get(h, 1.0) * p_of(k - 1, g[1:])

    for k in range(2, order + 1):
        tot, n1 = defaultdict(int), defaultdict(int)
        for g, c in counts[k - 1].items():
            tot[g[:-1]] += c
            n1[g[:-1]] += 1
        gamma.append({h: discount * n1[h] / tot[h] for h in tot})
        prob.append({})
        pk = {}
        for g, c in counts[k - 1].items():
            h = g[:-1]
            pk[g] = (c - discount) / tot[h] + gamma[k - 1][h] * p_of(k - 1, g[1:])
        prob[k - 1] = pk
    by_order = []
    for k in range(1, order + 1):
        rows = []
        if k == 1:
            nxt = gamma[1] if order > 1 else {}
            rows.append((("<s>",), -99.0, math.log10(nxt[("<s>",)]) if ("<s>",) in nxt else (0.0 if order > 1 else None)))
            for w in W:
                bo = None if order == 1 else (math.log10(nxt[(w,)]) if (w,) in nxt else 0.0)
                rows.append(((w,), math.log10(prob[0][(w,)]), bo))
        else:
            nxt = gamma[k] if k < order else {}
            for g in sorted(prob[k - 1]):
                bo = None if k == order else (math.log10(nxt[g]) if g in nxt else 0.0)
                rows.append((g, math.log10(prob[k - 1][g]), bo))
        by_order.append(rows)
    write_arpa(path, by_order)
    return by_order


def random_arpa(path, order, n_words, n_per_order, rng, with_unk=True):
    """Arbitrary log-probabilities (-6 .. -0.05) and back-offs (-2 .. 0.4, a quarter of them exactly 0); per order k >= 2
    about n_per_order n-grams: a random listed (k-1)-gram followed by a random word, so the set is closed under "context is
    listed".  -> the word list (without <s>, </s>, <unk>)."""
    words = [f"w{i}" for i in range(n_words)]
    uni = ["<s>", "</s>"] + (["<unk>"] if with_unk else []) + words
    last = uni[1:]                                          # <s> is never predicted

    def vals(n, bo):
        lp = rng.uniform(-6.0, -0.05, n)
        b = rng.uniform(-2.0, 0.4, n) * (rng.random(n) > 0.25)
        return lp, (b if bo else [None] * n)

    lp, b = vals(len(uni), order > 1)
    by_order = [[((w,), lp[i], b[i]) for i, w in enumerate(uni)]]
    prev = [(w,) for w in uni if w != "</s>"]               # nothing follows </s>
    for k in range(2, order + 1):
        pi = rng.integers(0, len(prev), n_per_order)
        wi = rng.integers(0, len(last), n_per_order)
        grams = sorted({prev[a] + (last[c],) for a, c in zip(pi, wi)})
        lp, b = vals(len(grams), k < order)
        by_order.append([(g, lp[i], b[i]) for i, g in enumerate(grams)])
        prev = [g for g in grams if g[-1] != "</s>"]
    write_arpa(path, by_order)
    return words
