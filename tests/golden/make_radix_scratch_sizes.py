#!/usr/bin/env python3
"""Generates tests/golden/radix_scratch_sizes.json: for every case of tests/test_radix_scratch_memory.py
(test_scratch_gives_back_what_it_took) the two numbers its scratch entry point returns, [real creation, size query], under
"emu" for the shapes of the CPU tier and under "hip" for the shapes of the MI355X.

The numbers are host-side sums of the bytes a scratch asks for, so both sets are computed on the host emulation; a size
query counts the index uploads and a real creation does not, which is why the two differ.

Recorded results only.  Run on the commit whose sizes are the reference, from the repository root:
    python tests/golden/make_radix_scratch_sizes.py
TFHE_EMU_LIB selects another build of the emulation library (the one of an earlier commit, for instance)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "radix_scratch_sizes.json")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import test_radix_scratch_memory as t
    from tests.harness import use_backend
    from tfhe_rs_amd import core_crypto_gpu as gpu
    from tfhe_rs_amd import integer_gpu as igpu
    lib = use_backend("emu")
    st = gpu.CudaStreams((0,))
    s, keep = igpu.CudaServerKey._streams(st)
    sizes = {}
    for shapes in ("emu", "hip"):
        sizes[shapes] = {}
        for name, case in t.scratch_cases(shapes).items():
            real, held = t.create_and_clean(lib, s, case, True)
            query, held_by_query = t.create_and_clean(lib, s, case, False)
            assert held > 0 and held_by_query == 0, name
            sizes[shapes][name] = [real, query]
            print(shapes, name, real, query)
    with open(OUT, "w") as f:
        json.dump(sizes, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
