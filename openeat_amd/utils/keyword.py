"""Host side of keyword search over CTC posteriors (ASRModel.keyword_search, ops.ctc_keyword_search; semantics in
include/openeat_hip.h, oe_ctc_kws): the keyword list with the tables the kernel reads, and the records made of its outputs.
No kernel here."""
import math
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

MAX_LABELS = 32                  # a state per lane of a wave: 2 * 32 - 1 = 63
MAX_KEYWORDS = 65535


class KeywordList:
    """KeywordList(phrases, threshold=0.5, thresholds=None): phrases = token-id sequences of 1 .. 32 labels each (blank, 0, is
    not a label); threshold = the confidence in (0, 1] a hit must reach - the geometric mean per frame of the posteriors on its
    path - for every keyword, or thresholds = one per keyword.  Kept as its natural log in float32, which is what the kernel
    compares against (`log_thr`).

    Host tables (oe_keyword_set): cols (U) int32 = the distinct tokens of all keywords, ascending; kw_col (K, Lmax) int32 = the
    index into cols of each label, 0 behind a keyword's end; klens (K) int32; log_thr (K) float32."""

    def __init__(self, phrases: Sequence[Sequence[int]], threshold: float = 0.5, thresholds: Optional[Sequence[float]] = None):
        self.phrases = [tuple(int(t) for t in p) for p in phrases]
        K = len(self.phrases)
        if not 1 <= K <= MAX_KEYWORDS:
            raise ValueError(f"KeywordList: {K} keywords outside 1 .. {MAX_KEYWORDS}")
        for p in self.phrases:
            if not 1 <= len(p) <= MAX_LABELS:
                raise ValueError(f"KeywordList: a keyword of {len(p)} labels outside 1 .. {MAX_LABELS}: {list(p)[:8]}")
        conf = [float(threshold)] * K if thresholds is None else [float(c) for c in thresholds]
        if len(conf) != K or not all(0.0 < c <= 1.0 for c in conf):
            raise ValueError("KeywordList: one threshold per keyword, each a confidence in (0, 1]")
        self.confidence = conf
        self.log_thr = np.log(np.asarray(conf, dtype=np.float64)).astype(np.float32)
        self.cols = np.asarray(sorted({t for p in self.phrases for t in p}), dtype=np.int32)
        index = {int(t): i for i, t in enumerate(self.cols)}
        self.klens = np.asarray([len(p) for p in self.phrases], dtype=np.int32)
        self.kw_col = np.zeros((K, int(self.klens.max())), dtype=np.int32)
        for k, p in enumerate(self.phrases):
            self.kw_col[k, : len(p)] = [index[t] for t in p]
        self.skipped = 0
        self._device: Dict[object, tuple] = {}

    def __len__(self):
        return len(self.phrases)

    @classmethod
    def from_text(cls, lines: Iterable[str], token2id, threshold: float = 0.5):
        """One keyword per line, split into the recipe's character tokens (every non-space character, as
        ContextGraph.from_text).  A line with a character token2id does not list (or maps to the blank), or of more than 32
        tokens, is skipped and counted in `.skipped`; empty lines and repeated keywords (the first is kept) are dropped."""
        phrases, seen, skipped = [], set(), 0
        for line in lines:
            chars = [ch for ch in line if not ch.isspace()]
            if not chars:
                continue
            ids = tuple(token2id.get(ch, 0) for ch in chars)
            if any(i <= 0 for i in ids) or len(ids) > MAX_LABELS:
                skipped += 1
                continue
            if ids not in seen:
                seen.add(ids)
                phrases.append(ids)
        self = cls(phrases, threshold)
        self.skipped = skipped
        return self

    def subset(self, lo: int, hi: int) -> "KeywordList":
        """The keywords lo .. hi-1 as a list of their own (its cols are their tokens only)."""
        return KeywordList(self.phrases[lo:hi], thresholds=self.confidence[lo:hi])

    def group_bounds(self, max_cols: int) -> List[int]:
        """Cut points [0, .., K] of consecutive groups whose distinct tokens number at most max_cols each (a single keyword with
        more forms a group of its own)."""
        bounds, seen = [0], set()
        for k, p in enumerate(self.phrases):
            new = seen | set(p)
            if len(new) > max_cols and k > bounds[-1]:
                bounds.append(k)
                new = set(p)
            seen = new
        bounds.append(len(self.phrases))
        return bounds

    def host_tables(self):
        """The arrays device_tables copies, as numpy."""
        return self.cols.copy(), self.kw_col.copy(), self.klens.copy(), self.log_thr.copy()

    def device_tables(self, device):
        """(cols (U) int32, kw_col (K, Lmax) int32, klens (K) int32, log_thr (K) float32) on `device`; made once per device and kept."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError(f"KeywordList: device tables live on a GPU (got {device})")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(device)
        if t is None:
            t = tuple(torch.from_numpy(a).to(device) for a in self.host_tables())
            self._device[device] = t
        return t


def hit_records(keywords: KeywordList, n_hits, hit_start, hit_end, hit_score, times=None):
    """The outputs of ops.ctc_keyword_search, already on the host as nested lists (n_hits (B, K); hit_* (B, K, max_hits)) ->
    (per recording the list of hits in time order, each {"keyword": index, "tokens", "start_frame", "end_frame" (inclusive),
    "score", "confidence" = exp(score / frames)}, and the truncation flags (B, K): n_hits > max_hits).  times: a function
    (start_frame, end_frame) -> (start_s, end_s) that adds "start_s" / "end_s"."""
    out, truncated = [], []
    for b, per_kw in enumerate(n_hits):
        recs, flags = [], []
        for k, n in enumerate(per_kw):
            stored = len(hit_start[b][k])
            flags.append(int(n) > stored)
            for i in range(min(int(n), stored)):
                s, e, sc = int(hit_start[b][k][i]), int(hit_end[b][k][i]), float(hit_score[b][k][i])
                rec = {"keyword": k, "tokens": list(keywords.phrases[k]), "start_frame": s, "end_frame": e, "score": sc,
                       "confidence": math.exp(sc / (e - s + 1))}
                if times is not None:
                    rec["start_s"], rec["end_s"] = times(s, e)
                recs.append(rec)
        recs.sort(key=lambda r: (r["start_frame"], r["end_frame"], r["keyword"]))
        out.append(recs)
        truncated.append(flags)
    return out, truncated
