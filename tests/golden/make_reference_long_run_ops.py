#!/usr/bin/env python3
"""Generates tests/golden/reference_long_run_ops.json: the operation NAMES of the reference's long-run tests of the radix
layer (integer/server_key/radix_parallel/tests_long_run/test_random_op_sequence.rs and its signed twin, and the GPU twins
of both under integer/gpu/server_key/radix/tests_long_run/), as the strings their operation tables pair with each
executor, plus the names of the ERC-7984 programs of test_erc7984.rs.

Names only.  The tests read the JSON, never the reference tree; tests/test_radix_op_sequence.py re-derives the lists with
`operation_names` where a tree is present.
Run where the reference tree is present:  python tests/golden/make_reference_long_run_ops.py <path to the tfhe-rs checkout>
(or with TFHE_RS_REFERENCE set)."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_long_run_ops.json")
CPU = "tfhe/src/integer/server_key/radix_parallel/tests_long_run"
GPU = "tfhe/src/integer/gpu/server_key/radix/tests_long_run"
SEQUENCES = {"unsigned": "test_random_op_sequence.rs", "signed": "test_signed_random_op_sequence.rs"}
NAME = re.compile(r'"([A-Za-z0-9_ ]+)"\s*\.to_string\(\)')
PROGRAM = re.compile(r"pub\(crate\) fn (\w+?)_erc7984_test\b")


def operation_names(root):
    """{"unsigned": [...], "signed": [...], "erc7984_programs": [...]}, each sorted; the union of a CPU file and its GPU
    twin (the GPU files add the OPRF forms that re-randomise)"""
    out = {}
    for kind, name in SEQUENCES.items():
        names = set()
        for folder in (CPU, GPU):
            with open(os.path.join(root, folder, name)) as f:
                names |= set(NAME.findall(f.read()))
        out[kind] = sorted(names)
    with open(os.path.join(root, CPU, "test_erc7984.rs")) as f:
        out["erc7984_programs"] = sorted(set(PROGRAM.findall(f.read())))
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TFHE_RS_REFERENCE")
    if not root:
        raise SystemExit(__doc__)
    names = operation_names(root)
    with open(OUT, "w") as f:
        json.dump(names, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in names.items()}, "->", OUT)


if __name__ == "__main__":
    main()
