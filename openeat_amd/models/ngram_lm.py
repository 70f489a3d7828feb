"""Back-off n-gram language model read from an ARPA file - the reference's default LM route into attention_rescoring
(the reference's openeat/bin/recognize.py:163-178: `kenlm.LanguageModel(args.lm)`; asr_model.py:515-516:
`lm.score(' '.join(content), bos=True, eos=True)`), without kenlm.

`NgramLM(arpa_path, token2char)` scores on the host with kenlm's call signature (`score`, `full_scores`: total / per-word
log10 probabilities) and, through `ops.ngram_score`, all hypotheses of a batch on the device (`oe_ngram_score`).  It is
deliberately not a torch.nn.Module: attention_rescoring tells a neural LM from an n-gram one by that.

The definition (ARPA back-off):  p(w | h) = logp(h w) if the n-gram `h w` is listed, else backoff(h) + p(w | h without its
first word), backoff(h) = 0 when h is not listed; h = the last order-1 words, from <s> when bos (context only), </s>
scored when eos.  A word the file does not list is <unk>; a file without an <unk> unigram gets one with log10 p = -100 and
back-off 0 (kenlm's default).  Values are float32 (`np.float32(float(text))`), sums float64.

Lookup structure (shared by host and device, layout in include/openeat_hip.h): every listed n-gram has an entry number - a
unigram's is its word id, a longer one's is n_words + its slot in ONE open-addressing table (linear probing, capacity a power
of two >= 2 x the n-grams of order >= 2) - and the key of a k-gram is (entry of its first k-1 words) << 32 | id of its k-th
word.  The key is the n-gram itself, so a lookup is exact; no hash value is ever taken for an n-gram.
"""
import numpy as np

MAX_ORDER = 5
UNK_LOGP = -100.0
_EMPTY = 0xFFFFFFFFFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
_C1, _C2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53


def _mix(x: np.ndarray) -> np.ndarray:
    """murmur3's 64-bit finaliser on a uint64 array (wraps modulo 2^64)."""
    x = x.copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(_C1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(_C2)
    x ^= x >> np.uint64(33)
    return x


def _mix_int(x: int) -> int:
    x ^= x >> 33
    x = (x * _C1) & _M64
    x ^= x >> 33
    x = (x * _C2) & _M64
    x ^= x >> 33
    return x


def read_arpa(path, max_order: int = MAX_ORDER):
    """-> (vocab: word strings by id, in the order of the 1-gram section; orders: for k = 1.. a tuple (ids (M, k) int32,
    logp (M) float32, backoff (M) float32, line numbers (M) int64)).  ValueError with the line number on anything malformed."""
    counts, vocab, word_id = {}, [], {}
    rows = []                                                      # per order: [ids], [logp], [bo], [line]
    section, seen_data, ended, lineno = None, False, False, 0

    def close_section(at):
        if section is not None and len(rows[section - 1][1]) != counts[section]:
            raise ValueError(f"{path}:{at}: \\{section}-grams: has {len(rows[section - 1][1])} entries, the header says {counts[section]}")

    with open(path, "r", encoding="utf-8") as f:
        for lineno, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            if ended:
                raise ValueError(f"{path}:{lineno}: text after \\end\\")
            if line[0] == "\\":
                if line == "\\data\\":
                    seen_data = True
                elif line == "\\end\\":
                    close_section(lineno)
                    if section is None or section != max(counts):
                        raise ValueError(f"{path}:{lineno}: \\end\\ before every announced section was read")
                    ended = True
                elif line.endswith("-grams:") and line[1:-7].isdigit():
                    close_section(lineno)
                    k = int(line[1:-7])
                    if k not in counts or k != (section or 0) + 1:
                        raise ValueError(f"{path}:{lineno}: unexpected section {line}")
                    section = k
                else:
                    raise ValueError(f"{path}:{lineno}: unknown directive {line}")
                continue
            if section is None:
                if seen_data and line.startswith("ngram ") and "=" in line:
                    k, c = line[6:].split("=", 1)
                    k, c = int(k), int(c)
                    if k > max_order:
                        raise ValueError(f"{path}:{lineno}: order {k} is above the supported maximum {max_order}")
                    if k != len(counts) + 1:
                        raise ValueError(f"{path}:{lineno}: orders must be announced as 1, 2, ..")
                    counts[k] = c
                    rows.append(([], [], [], []))
                    continue
                raise ValueError(f"{path}:{lineno}: expected \\data\\ and 'ngram N=count' lines")
            fields = line.split()
            k = section
            if len(fields) not in (k + 1, k + 2):
                raise ValueError(f"{path}:{lineno}: a {k}-gram line has a log-probability, {k} words and at most a back-off")
            try:
                lp = np.float32(float(fields[0]))
                bo = np.float32(float(fields[k + 1])) if len(fields) == k + 2 else np.float32(0.0)
            except ValueError:
                raise ValueError(f"{path}:{lineno}: not a number") from None
            if k == 1:
                if fields[1] in word_id:
                    raise ValueError(f"{path}:{lineno}: word {fields[1]!r} listed twice")
                word_id[fields[1]] = len(vocab)
                vocab.append(fields[1])
                ids = (word_id[fields[1]],)
            else:
                try:
                    ids = tuple(word_id[w] for w in fields[1:k + 1])
                except KeyError as e:
                    raise ValueError(f"{path}:{lineno}: word {e.args[0]!r} is not in the 1-gram section") from None
            r = rows[k - 1]
            r[0].append(ids); r[1].append(lp); r[2].append(bo); r[3].append(lineno)
    if not ended:
        raise ValueError(f"{path}:{lineno}: missing \\end\\")
    orders = []
    for k, r in enumerate(rows, 1):
        orders.append((np.asarray(r[0], dtype=np.int32).reshape(-1, k), np.asarray(r[1], dtype=np.float32),
                       np.asarray(r[2], dtype=np.float32), np.asarray(r[3], dtype=np.int64)))
    return vocab, orders


class NgramLM:
    """n-gram LM over the strings of `token2char` (id -> string; a dict or a list).  Host: `score`, `full_scores`.  Device:
    `ops.ngram_score(lm, tokens, lens)` / `attention_rescoring_batch(lm=..., lm_weight=...)`; the device tables are made on
    first device use (or by `.to(device)`), owned by this object and never rebuilt (captured launches point at them)."""

    def __init__(self, arpa_path, token2char):
        vocab, orders = read_arpa(arpa_path)
        self._init(vocab, orders, token2char, str(arpa_path))

    @classmethod
    def from_arrays(cls, vocab, orders, token2char):
        """From what read_arpa returns (synthetic models, e.g. tools/ngram_bench.py) - the same checks, no file."""
        self = cls.__new__(cls)
        self._init(list(vocab), orders, token2char, "<arrays>")
        return self

    # ------------------------------------------------------------------ construction
    def _init(self, vocab, orders, token2char, where):
        if not orders or len(orders) > MAX_ORDER:
            raise ValueError(f"{where}: orders 1..{MAX_ORDER} are supported")
        word_id = {w: i for i, w in enumerate(vocab)}
        for special in ("<s>", "</s>"):
            if special not in word_id:
                raise ValueError(f"{where}: the 1-gram section does not list {special}")
        uni_lp, uni_bo = orders[0][1].astype(np.float32), orders[0][2].astype(np.float32)
        if "<unk>" not in word_id:
            word_id["<unk>"] = len(vocab)
            vocab = vocab + ["<unk>"]
            uni_lp = np.append(uni_lp, np.float32(UNK_LOGP))
            uni_bo = np.append(uni_bo, np.float32(0.0))
        self.order = len(orders)
        self.vocab, self.word_id = vocab, word_id
        self.n_words = len(vocab)
        self.bos_word, self.eos_word, self.unk_word = word_id["<s>"], word_id["</s>"], word_id["<unk>"]
        self.unigrams = np.ascontiguousarray(np.stack([uni_lp, uni_bo], 1))             # (n_words, 2) float32
        n_high = sum(len(o[1]) for o in orders[1:])
        cap = 2
        while cap < 2 * n_high:
            cap *= 2
        if self.n_words + cap >= 2 ** 31:
            raise ValueError(f"{where}: too many n-grams for 31-bit entry numbers")
        self.capacity, self.max_probe, self.n_ngrams = cap, 0, self.n_words + n_high
        self._table = np.zeros(cap, dtype=np.dtype([("key", "<u8"), ("logp", "<f4"), ("backoff", "<f4")]))
        self._table["key"] = np.uint64(_EMPTY)
        for k in range(2, self.order + 1):
            ids, lp, bo, lines = orders[k - 1]
            if len(lp) == 0:
                continue
            ent = ids[:, 0].astype(np.int64)
            for j in range(1, k - 1):                                               # entry of the first k-1 words
                ent = self._find_many(ent, ids[:, j])
            if (ent < 0).any():
                i = int(np.argmax(ent < 0))
                raise ValueError(f"{where}:{int(lines[i])}: the context of this {k}-gram (its first {k - 1} words) is not listed")
            keys = (ent.astype(np.uint64) << np.uint64(32)) | ids[:, k - 1].astype(np.uint64)
            srt = np.argsort(keys, kind="stable")
            dup = np.nonzero(keys[srt][1:] == keys[srt][:-1])[0]
            if dup.size:
                raise ValueError(f"{where}:{int(lines[srt[dup[0] + 1]])}: this {k}-gram is listed twice")
            slots = self._insert(keys)
            self._table["logp"][slots] = lp
            self._table["backoff"][slots] = bo
        self._bind_tokens(token2char)
        self._device = {}

    def _insert(self, keys):
        """Linear-probing insert of distinct new keys, all at once: in every round each pending key looks at its slot; of
        the keys that meet the same empty slot the first takes it, everyone else moves one slot on."""
        tab = self._table["key"]
        mask = np.uint64(self.capacity - 1)
        slot = _mix(keys) & mask
        out = np.empty(len(keys), dtype=np.int64)
        pending = np.arange(len(keys))
        dist = 0
        while pending.size:
            s = slot[pending]
            free = tab[s] == np.uint64(_EMPTY)
            cand, cs = pending[free], s[free]
            u, first = np.unique(cs, return_index=True)
            win = cand[first]
            tab[u] = keys[win]
            out[win] = u.astype(np.int64)
            placed = np.zeros(len(keys), dtype=bool)
            placed[win] = True
            pending = pending[~placed[pending]]
            if pending.size:
                slot[pending] = (slot[pending] + np.uint64(1)) & mask
                dist += 1
                self.max_probe = max(self.max_probe, dist)
        return out

    def _find_many(self, ent, word):
        """Entry numbers of the n-grams (entry `ent`, then `word`), -1 where not listed (or ent < 0)."""
        tab = self._table["key"]
        mask = np.uint64(self.capacity - 1)
        res = np.full(len(ent), -1, dtype=np.int64)
        act = np.nonzero(ent >= 0)[0]
        keys = (ent[act].astype(np.uint64) << np.uint64(32)) | word[act].astype(np.uint64)
        slot = _mix(keys) & mask
        for _ in range(self.max_probe + 1):
            if act.size == 0:
                break
            k = tab[slot]
            hit = k == keys
            res[act[hit]] = self.n_words + slot[hit].astype(np.int64)
            go = ~hit & (k != np.uint64(_EMPTY))
            act, keys, slot = act[go], keys[go], (slot[go] + np.uint64(1)) & mask
        return res

    def _bind_tokens(self, token2char):
        items = list(token2char.items()) if isinstance(token2char, dict) else list(enumerate(token2char))
        V = (max(int(t) for t, _ in items) + 1) if items else 1
        tok2word = np.full(V, self.unk_word, dtype=np.int32)
        for t, s in items:
            if not isinstance(s, str) or len(s.split()) != 1 or s != s.strip():
                raise ValueError(f"token {t}: the string {s!r} is empty or contains whitespace; joined with spaces it would not be "
                                 "one LM word (multi-word tokens are not supported)")
            if int(t) < 0:
                raise ValueError(f"token id {t} is negative")
            tok2word[int(t)] = self.word_id.get(s, self.unk_word)
        self.token2char = token2char
        self.tok2word = tok2word

    # ------------------------------------------------------------------ host scoring (kenlm's signatures)
    def _find(self, ent: int, word: int) -> int:
        key = (ent << 32) | word
        tab = self._table["key"]
        mask = self.capacity - 1
        slot = _mix_int(key) & mask
        for _ in range(self.max_probe + 1):
            k = int(tab[slot])
            if k == key:
                return slot
            if k == _EMPTY:
                return -1
            slot = (slot + 1) & mask
        return -1

    def full_scores(self, sentence: str, bos: bool = True, eos: bool = True):
        """Per word of the sentence (and </s> when eos): (log10 p, length of the matched n-gram, is_oov)."""
        words = sentence.split()
        ids = [self.word_id.get(w) for w in words]
        oov = [i is None for i in ids] + [False]
        seq = ([self.bos_word] if bos else []) + [self.unk_word if i is None else i for i in ids] + ([self.eos_word] if eos else [])
        off = 1 if bos else 0
        chains = []                                            # chains[s][k-1] = (log10 p, back-off) of seq[s : s + k], while listed
        for s in range(len(seq)):
            ent = seq[s]
            ch = [(self.unigrams[ent, 0], self.unigrams[ent, 1])]
            for k in range(2, self.order + 1):
                if s + k - 1 >= len(seq):
                    break
                slot = self._find(ent, seq[s + k - 1])
                if slot < 0:
                    break
                ch.append((self._table["logp"][slot], self._table["backoff"][slot]))
                ent = self.n_words + slot
            chains.append(ch)
        out = []
        for i in range(off, len(seq)):
            term, k = 0.0, min(self.order, i + 1)
            while k > 1:
                ch = chains[i - k + 1]
                if len(ch) >= k:
                    break
                if len(ch) >= k - 1:
                    term += float(ch[k - 2][1])
                k -= 1
            term += float(chains[i - k + 1][k - 1][0])
            out.append((term, k, oov[i - off]))
        return out

    def score(self, sentence: str, bos: bool = True, eos: bool = True) -> float:
        """Total log10 probability of the sentence (words split on whitespace)."""
        return float(sum(t for t, _, _ in self.full_scores(sentence, bos, eos)))

    # ------------------------------------------------------------------ device tables
    def to(self, device):
        self.device_tables(device)
        return self

    def device_tables(self, device):
        """(unigrams (n_words, 2) float32, table (capacity, 4) int32 = the 16-byte slots, tok2word (V) int32) on `device`;
        made once per device and kept."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError(f"NgramLM: device tables live on a GPU (got {device}); on the host use score / full_scores")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(device)
        if t is None:
            t = (torch.from_numpy(self.unigrams).to(device),
                 torch.from_numpy(self._table.view(np.int32).reshape(self.capacity, 4)).to(device),
                 torch.from_numpy(self.tok2word).to(device))
            self._device[device] = t
        return t
