#!/usr/bin/env python3
"""Writes tests/golden/pairing_constants.json: the Frobenius coefficients of BLS12-377's Fq6 and Fq12 as the reference's parameter files
state them (curves/bls12_377/src/fields/fq6.rs:17-69, fq12.rs:15-73), parsed from the text into integers, plus the SHA-256 of each file.
Run where the reference tree is readable:  python tests/golden/make_pairing_constants.py [REFERENCE_ROOT]"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pairing_constants.json")
FILES = {"fq6": "curves/bls12_377/src/fields/fq6.rs", "fq12": "curves/bls12_377/src/fields/fq12.rs"}
NAMES = {"fq6": ("FROBENIUS_COEFF_FP6_C1", "FROBENIUS_COEFF_FP6_C2"), "fq12": ("FROBENIUS_COEFF_FP12_C1",)}
Q = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
_TOKEN = re.compile(r'FQ_ONE|FQ_ZERO|field_new!\(\s*Fq\s*,\s*"(-?\d+)"\s*\)')


def parse_coefficients(text: str, name: str):
    """The Fq2 array `name` of a parameter file: [[c0, c1], ...] as canonical integers (comments ignored)."""
    text = re.sub(r"//[^\n]*", "", text)
    m = re.search(r"const\s+" + name + r"\s*:[^=]*=\s*&\[(.*?)\];", text, re.S)
    assert m, name
    vals = []
    for t in _TOKEN.finditer(m.group(1)):
        if t.group(0) == "FQ_ONE":
            vals.append(1)
        elif t.group(0) == "FQ_ZERO":
            vals.append(0)
        else:
            vals.append(int(t.group(1)) % Q)
    assert len(vals) % 2 == 0, name
    return [[vals[i], vals[i + 1]] for i in range(0, len(vals), 2)]


def read_reference(root: str) -> dict:
    out, sha = {}, {}
    for key, rel in FILES.items():
        raw = open(os.path.join(root, rel), "rb").read()
        sha[rel] = hashlib.sha256(raw).hexdigest()
        for name in NAMES[key]:
            out[name] = parse_coefficients(raw.decode(), name)
    out["_sha256"] = sha
    return out


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    d = read_reference(root)
    json.dump({k: ([[str(a), str(b)] for a, b in v] if not k.startswith("_") else v) for k, v in d.items()}, open(OUT, "w"), indent=1)
    print(OUT)
