#!/usr/bin/env python3
"""Writes tests/golden/f26_edit_distance.json: what the reference's error-rate tool answers on fixed-seed token pairs.

  python tests/golden/make_edit_distance_fixture.py <path to the reference's tools/compute-wer.py>

The tool is loaded from that path at generation time only; nothing of it is kept here.  Every record holds the two token
sequences and the `all / cor / sub / del / ins` of `Calculator().calculate(ref, hyp)`.  Vocabularies of 2, 3, 5 and 50
symbols (small ones make ties dense), lengths from {0, 1, 2, 5, 17, 40} in every order, both-empty included, two draws per
combination: 288 pairs."""
import importlib.util
import json
import os
import random
import sys

VOCABS = (2, 3, 5, 50)
LENGTHS = (0, 1, 2, 5, 17, 40)
DRAWS = 2


def main():
    spec = importlib.util.spec_from_file_location("compute_wer", sys.argv[1])
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = random.Random(26)
    records = []
    for vocab in VOCABS:
        for n in LENGTHS:
            for m in LENGTHS:
                for _ in range(DRAWS):
                    ref = [rng.randrange(vocab) for _ in range(n)]
                    hyp = [rng.randrange(vocab) for _ in range(m)]
                    # the tool works on non-empty strings and prepends to the lists it is given
                    res = tool.Calculator().calculate(["t%d" % t for t in ref], ["t%d" % t for t in hyp])
                    records.append({"vocab": vocab, "ref": ref, "hyp": hyp, "all": res["all"], "cor": res["cor"], "sub": res["sub"],
                                    "del": res["del"], "ins": res["ins"]})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "f26_edit_distance.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in records) + "\n]\n")
    print(f"wrote {len(records)} records to {out}")


if __name__ == "__main__":
    main()
