#!/usr/bin/env python3
"""Writes tests/golden/reference_line_counts.json: the line count and SHA-256 of every reference source file that
tests/golden/plonk_marlin_callsites.json cites (DATA only: paths and numbers, no source text).  tests/test_callsite_audit.py
checks the citations against this index on any machine, and against the reference tree itself where one is present.

    python tests/golden/make_reference_index.py <reference root>
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_line_counts.json")


def cited_files() -> list:
    spec = json.load(open(os.path.join(HERE, "plonk_marlin_callsites.json")))
    return sorted({path for prover in ("plonk", "marlin") for site in spec[prover]["sites"]
                   for path, _ in re.findall(r"([\w\-/\.]+\.rs):(\d+)", site["ref"])})


def index(root: str) -> dict:
    out = {}
    for rel in cited_files():
        data = open(os.path.join(root, rel), "rb").read()
        out[rel] = {"lines": data.count(b"\n") + (0 if data.endswith(b"\n") or not data else 1), "sha256": hashlib.sha256(data).hexdigest()}
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    json.dump({"_source": "alex-ozdemir/collaborative-zksnark (indexed by tests/golden/make_reference_index.py)", "files": index(sys.argv[1])},
              open(OUT, "w"), indent=1, sort_keys=True)
    print("wrote", OUT)
