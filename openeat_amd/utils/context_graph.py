"""Hotword (contextual) biasing for the device CTC prefix beam search: the host builder of the context graph that
`oe_ctc_prefix_beam` reads (semantics in include/openeat_hip.h, restated here).

A graph is a set of distinct phrases q (1..32 token ids >= 1, never the blank), each with a float32 score s(q), and one
float32 per-token partial credit c >= 0; by default s(q) = c * len(q) in float32.  For a token prefix p
    hits(p) = the sum of s(q) over every occurrence of every phrase in p - overlapping and nested ones all count - the
              float32 values added in float64 by increasing end position, the longest phrase first within one position;
    k(p)    = the largest k <= len(p) such that the last k tokens of p are a PROPER prefix of some phrase (0: none);
    bias(p) = hits(p) + float64(c) * k(p) during the search, hits(p) with final=True (the pending credit is dropped).

The automaton (Aho-Corasick): states are trie nodes, the root is 0, numbered breadth first.
    fail[s]   the longest proper suffix of s that is a trie node (0 for the root);
    out[s]    = (score, link): score the float32 s(q) of the phrase that ends exactly at s (0.0: none ends here - adding it
              changes no bit), link the nearest state on s's fail chain at which a phrase ends (0: none).  The phrases that
              end at s are a LIST, s, link[s], link[link[s]], .. - longest first, at most 32 - and not a pre-summed value:
              (h + a) + b is the stated float64 sum, h + (a + b) is not.
    pend[s]   the depth of the first node on s, fail[s], .. that has children: k(p) for a prefix that sits in s.
Only the trie's edges are stored (size linear in the total phrase length); a missing edge follows fail[] (at most 32 steps,
33 probes; none for a prefix that sits in the root and leaves it or stays).  The edges use the n-gram table's format (ngram_lm.py,
ngram_common.h): 16-byte slots {u64 key, i32 next state, i32 0}, key = state << 32 | token, open addressing with linear
probing from murmur3_fmix64(key) & (capacity - 1), empty key = ~0, capacity a power of two >= twice the edges, max_probe the
longest displacement.
"""
from collections import deque

import numpy as np

from openeat_amd.models.ngram_lm import _EMPTY, _mix_int

MAX_PHRASE = 32
MAX_STATES = 1 << 20


class ContextGraph:
    """ContextGraph(phrases, context_score=3.0, phrase_scores=None): phrases = token-id sequences; phrase_scores = one score
    per phrase instead of context_score * length.  Host: `bias(prefix, final)`.  Device: `device_tables(device)`, made on
    first use per device, owned by this object and never rebuilt (captured launches point at them)."""

    def __init__(self, phrases, context_score: float = 3.0, phrase_scores=None):
        phrases = [tuple(int(t) for t in q) for q in phrases]
        c = np.float32(context_score)
        if not np.isfinite(c) or c < 0:
            raise ValueError(f"context_score must be finite and >= 0 (got {context_score})")
        if phrase_scores is None:
            scores = [c * np.float32(len(q)) for q in phrases]
        else:
            if len(phrase_scores) != len(phrases):
                raise ValueError(f"{len(phrase_scores)} phrase_scores for {len(phrases)} phrases")
            scores = [np.float32(s) for s in phrase_scores]
        if not all(np.isfinite(s) for s in scores):
            raise ValueError("phrase scores must be finite")
        self.context_score = c
        self.phrases = phrases
        self.phrase_scores = np.asarray(scores, dtype=np.float32)
        self.skipped = 0

        children = [{}]                                                # per state: token -> state (insertion numbering)
        depth, score, ends = [0], [np.float32(0.0)], [False]
        for n, q in enumerate(phrases):
            if not 1 <= len(q) <= MAX_PHRASE:
                raise ValueError(f"phrase {n}: {len(q)} tokens; a phrase has 1..{MAX_PHRASE}")
            s = 0
            for t in q:
                if not 1 <= t < 2 ** 31:
                    raise ValueError(f"phrase {n}: token id {t}; ids are 1..V-1, never the blank")
                nxt = children[s].get(t)
                if nxt is None:
                    nxt = len(children)
                    if nxt >= MAX_STATES:
                        raise ValueError(f"more than {MAX_STATES} states")
                    children[s][t] = nxt
                    children.append({})
                    depth.append(depth[s] + 1); score.append(np.float32(0.0)); ends.append(False)
                s = nxt
            if ends[s]:
                raise ValueError(f"phrase {n} {q} is listed twice")
            ends[s], score[s] = True, scores[n]
        # breadth-first renumbering: a state's fail, link and pend targets are numbered below it
        order, new_id = [0], {0: 0}
        queue = deque([0])
        while queue:
            s = queue.popleft()
            for t, nxt in children[s].items():
                new_id[nxt] = len(order)
                order.append(nxt)
                queue.append(nxt)
        n_states = len(order)
        self.n_states = n_states
        self.depth = np.asarray([depth[s] for s in order], dtype=np.int32)
        self.score = np.asarray([score[s] for s in order], dtype=np.float32)
        self.ends = np.asarray([ends[s] for s in order], dtype=bool)
        self._edges = [{t: new_id[nxt] for t, nxt in children[s].items()} for s in order]
        self.fail = np.zeros(n_states, dtype=np.int32)
        self.link = np.zeros(n_states, dtype=np.int32)
        self.pend = np.zeros(n_states, dtype=np.int32)
        for s in range(n_states):                                      # parents come before children
            if s and not self._edges[s]:
                self.pend[s] = self.pend[self.fail[s]]
            elif s:
                self.pend[s] = self.depth[s]
            for t, nxt in self._edges[s].items():
                f = 0
                if s:
                    f = int(self.fail[s])
                    while f and t not in self._edges[f]:
                        f = int(self.fail[f])
                    f = self._edges[f].get(t, 0)
                self.fail[nxt] = f
                self.link[nxt] = f if self.ends[f] else self.link[f]
        self._build_table()
        self._device = {}

    @classmethod
    def from_text(cls, lines, token2id, context_score: float = 3.0):
        """One phrase per line, split into the recipe's character tokens (every non-space character, as the manifest reader
        does).  A line with a character token2id does not list (or maps to the blank) is skipped and counted in `.skipped`;
        empty lines and repeated phrases (the first is kept) are dropped silently."""
        phrases, seen, skipped = [], set(), 0
        for line in lines:
            chars = [ch for ch in line if not ch.isspace()]
            if not chars:
                continue
            ids = tuple(token2id.get(ch, 0) for ch in chars)
            if any(i <= 0 for i in ids):
                skipped += 1
                continue
            if ids not in seen:
                seen.add(ids)
                phrases.append(ids)
        self = cls(phrases, context_score)
        self.skipped = skipped
        return self

    # ------------------------------------------------------------------ the edge table
    def _build_table(self):
        n_edges = self.n_states - 1
        cap = 2
        while cap < 2 * n_edges:
            cap *= 2
        self.capacity, self.max_probe = cap, 0
        self._table = np.zeros(cap, dtype=np.dtype([("key", "<u8"), ("next", "<i4"), ("pad", "<i4")]))
        self._table["key"] = np.uint64(_EMPTY)
        keys = self._table["key"]
        mask = cap - 1
        for s, edges in enumerate(self._edges):
            for t, nxt in edges.items():
                key = (s << 32) | t
                slot, dist = _mix_int(key) & mask, 0
                while int(keys[slot]) != _EMPTY:
                    slot, dist = (slot + 1) & mask, dist + 1
                keys[slot] = np.uint64(key)
                self._table["next"][slot] = nxt
                self.max_probe = max(self.max_probe, dist)

    def _find(self, state: int, tok: int) -> int:
        """The edge (state, tok) through the table, as the device looks it up: the next state or -1."""
        key = (state << 32) | (tok & 0xFFFFFFFF)
        keys = self._table["key"]
        mask = self.capacity - 1
        slot = _mix_int(key) & mask
        for _ in range(self.max_probe + 1):
            k = int(keys[slot])
            if k == key:
                return int(self._table["next"][slot])
            if k == _EMPTY:
                return -1
            slot = (slot + 1) & mask
        return -1

    # ------------------------------------------------------------------ host walk
    def step(self, state: int, tok: int) -> int:
        """The state of prefix + [tok] for a prefix that sits in `state`."""
        while True:
            nxt = self._find(state, tok)
            if nxt >= 0:
                return nxt
            if state == 0:
                return 0
            state = int(self.fail[state])

    def bias(self, prefix, final: bool = False) -> float:
        """bias(prefix) as the search adds it (module docstring); final: the pending credit is dropped."""
        s, hits = 0, 0.0
        for tok in prefix:
            s = self.step(s, int(tok))
            t = s
            while t:
                hits += float(self.score[t])
                t = int(self.link[t])
        return hits if final else hits + float(self.context_score) * int(self.pend[s])

    # ------------------------------------------------------------------ device tables
    def device_tables(self, device):
        """(edges (capacity, 4) int32 = the 16-byte slots, fail (n_states) int32, out (n_states, 2) int32 = (score bits,
        link), pend (n_states) int32) on `device`; made once per device and kept."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError(f"ContextGraph: device tables live on a GPU (got {device}); on the host use bias")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(device)
        if t is None:
            t = tuple(torch.from_numpy(a).to(device) for a in self.host_tables())
            self._device[device] = t
        return t

    def host_tables(self):
        """The arrays device_tables copies, as numpy."""
        out = np.stack([self.score.view(np.int32), self.link], 1)
        return (self._table.view(np.int32).reshape(self.capacity, 4), self.fail.copy(), np.ascontiguousarray(out), self.pend.copy())
