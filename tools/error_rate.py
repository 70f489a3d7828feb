#!/usr/bin/env python3
"""Token error rate of a decode against its references, scored on the device (oe_edit_distance).

  python tools/error_rate.py ref.txt hyp.txt [--device cuda]

Both files hold one utterance per line, `key tok tok ...` (what the decode CLI writes).  Tokens are whitespace-separated
strings, compared as they stand; utterances are matched by key, and a key of ref.txt that hyp.txt does not have is reported
and skipped.  Prints the overall line of the reference's tools/compute-wer.py (`Overall -> 6.22 % N=.. C=.. S=.. D=.. I=..`)
with the same counts (semantics and tie order: include/openeat_hip.h).

Not done here: splitting into characters, case folding, dropping <tags> or ignore lists - prepare the files with the
reference's tool chain for that, or score with compute-wer.py itself.  Utterances longer than 1023 tokens are refused."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openeat_amd import ops  # noqa: E402
from openeat_amd.utils.error_rate import ErrorRate  # noqa: E402

CHUNK = 4096                                     # pairs per launch


def read(path):
    out = {}
    with open(path, encoding="utf-8") as f:
        for line in f:
            parts = line.split()
            if parts:
                out[parts[0]] = parts[1:]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ref")
    ap.add_argument("hyp")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    refs, hyps = read(a.ref), read(a.hyp)
    ids = {}                                     # token string -> id, in order of first appearance
    pairs = []
    for key, r in refs.items():
        if key not in hyps:
            print(f"no hypothesis for {key}: skipped", file=sys.stderr)
            continue
        pairs.append(([ids.setdefault(t, len(ids)) for t in r], [ids.setdefault(t, len(ids)) for t in hyps[key]]))
    er = ErrorRate()
    for c0 in range(0, len(pairs), CHUNK):
        chunk = pairs[c0:c0 + CHUNK]
        mats = []
        for side in (0, 1):
            lens = torch.tensor([len(p[side]) for p in chunk], dtype=torch.int32)
            mat = torch.zeros(len(chunk), max(int(lens.max()), 1), dtype=torch.int32)
            for k, p in enumerate(chunk):
                mat[k, : len(p[side])] = torch.tensor(p[side], dtype=torch.int32)
            mats += [mat.to(a.device), lens.to(a.device)]
        er.update(ops.edit_distance(*mats))
    print(er)


if __name__ == "__main__":
    main()
