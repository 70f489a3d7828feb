"""Plain-Python restatement of the edit distance oe_edit_distance computes (the semantics are written out in
include/openeat_hip.h; they are Calculator.calculate of the reference's tools/compute-wer.py, which
tests/golden/f26_edit_distance.json records).  The whole table of chosen predecessors is kept and walked back from (n, m):
the counts come from the back-trace, not from anything carried forward, so the device's counts-only path is checked
against a different derivation.  Independent of the code under test."""

DEL, INS, DIAG = 0, 1, 2


def edit_distance(ref, hyp):
    """ref, hyp: sequences of token ids -> ((cor, sub, del, ins), ref_to_hyp) with ref_to_hyp[i] the hypothesis position
    aligned with reference token i (cor or sub) or -1 if it is deleted."""
    r, h = list(ref), list(hyp)
    n, m = len(r), len(h)
    moves = [None] * (n + 1)
    prev = list(range(m + 1))                       # D[0][j] = j: all insertions
    for i in range(1, n + 1):
        ri = r[i - 1]
        cur = [i] * (m + 1)                         # D[i][0] = i: all deletions
        row = bytearray(m + 1)
        left = i
        for j in range(1, m + 1):
            best, mv = prev[j] + 1, DEL             # deletion first
            d = left + 1
            if d < best:                            # insertion only if strictly smaller
                best, mv = d, INS
            d = prev[j - 1] + (0 if ri == h[j - 1] else 1)
            if d < best:                            # diagonal only if strictly smaller
                best, mv = d, DIAG
            cur[j] = left = best
            row[j] = mv
        moves[i] = row
        prev = cur
    cor = sub = dele = ins = 0
    ref_to_hyp = [-1] * n
    i, j = n, m
    while i > 0 or j > 0:
        mv = INS if i == 0 else DEL if j == 0 else moves[i][j]
        if mv == DEL:
            dele += 1
            i -= 1
        elif mv == INS:
            ins += 1
            j -= 1
        else:
            if r[i - 1] == h[j - 1]:
                cor += 1
            else:
                sub += 1
            ref_to_hyp[i - 1] = j - 1
            i -= 1
            j -= 1
    return (cor, sub, dele, ins), ref_to_hyp
