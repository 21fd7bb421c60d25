#!/usr/bin/env python3
"""Generates tests/golden/reference_compression_sets.json: one entry per CompressionParameters constant the reference
defines under tfhe/src/shortint/parameters/**/list_compression* (the 64-bit ciphertext compression; the
NoiseSquashingCompressionParameters of the 128-bit path are a different type and stay out).  Per entry: name, file:line,
the decompression bootstrap's decomposition, the packing keyswitch's decomposition and GLWE, lwe_per_glwe, the storage
width, the noise field, and whether the set is a classic one or a GPU multi-bit one with its grouping factor
(the decompression_grouping_factor field where the constant has one, the GROUP_<g> of its name otherwise: the earlier
versions declare the GPU multi-bit sets with the classic struct and pair them with a multi-bit compute set by name).

Settings and names only.  The tests read the JSON, never the reference tree.
Run where the reference tree is present:  python tests/golden/make_compression_sets.py <path to the tfhe-rs checkout>
(or with TFHE_RS_REFERENCE set)."""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_compression_sets.json")
PARAMS = "tfhe/src/shortint/parameters"

CONST = re.compile(r"pub const (\w+)\s*:\s*CompressionParameters\s*=\s*(?:CompressionParameters::(Classic|MultiBit)\(\s*\w+|"
                   r"CompressionParameters)\s*\{(.*?)\n\s*\}\)?;", re.S)
NUMBER = {"br_level": "DecompositionLevelCount", "br_base_log": "DecompositionBaseLog",
          "packing_ks_level": "DecompositionLevelCount", "packing_ks_base_log": "DecompositionBaseLog",
          "packing_ks_polynomial_size": "PolynomialSize", "packing_ks_glwe_dimension": "GlweDimension",
          "lwe_per_glwe": "LweCiphertextCount", "storage_log_modulus": "CiphertextModulusLog"}


def noise_setting(text, rel, name):
    """the noise field as settings: {"distribution": "t_uniform", "bound_log2": b} or {"distribution": "gaussian", "std_dev": s}"""
    text = re.sub(r"\s+", "", text)
    m = re.fullmatch(r"DynamicDistribution::new_t_uniform\((\d+)\)", text)
    if m:
        return {"distribution": "t_uniform", "bound_log2": int(m.group(1))}
    m = re.fullmatch(r"DynamicDistribution::new_gaussian_from_std_dev\(StandardDev\(([0-9.eE+-]+),?\),?\)", text)
    if m:
        return {"distribution": "gaussian", "std_dev": float(m.group(1))}
    raise SystemExit(f"{rel}: {name}: noise field not understood: {text}")


def parse_file(path, rel):
    text = open(path).read()
    out = []
    for m in CONST.finditer(text):
        name, variant, body = m.group(1), m.group(2) or "Classic", m.group(3)
        e = {"name": name, "where": f"{rel}:{text.count(chr(10), 0, m.start()) + 1}", "struct": variant}
        for field, wrapper in NUMBER.items():
            f = re.search(rf"\b{field}:\s*{wrapper}\((\d+)\)", body)
            if not f:
                raise SystemExit(f"{rel}: {name} has no {field}")
            e[field] = int(f.group(1))
        noise = re.search(r"packing_ks_key_noise_distribution:\s*(.*?),\s*(?:decompression_grouping_factor|$)", body, re.S)
        if not noise:
            raise SystemExit(f"{rel}: {name} has no noise field")
        e["packing_ks_key_noise_distribution"] = noise_setting(noise.group(1), rel, name)
        g = re.search(r"decompression_grouping_factor:\s*LweBskGroupingFactor\((\d+)\)", body)
        by_name = re.search(r"GPU_MULTI_BIT_GROUP_(\d+)", name)
        if (variant == "MultiBit") != bool(g):
            raise SystemExit(f"{rel}: {name}: struct {variant} and grouping field disagree")
        if g and (not by_name or by_name.group(1) != g.group(1)):
            raise SystemExit(f"{rel}: {name}: grouping field {g.group(1)} is not the one of the name")
        e["kind"] = "gpu_multi_bit" if by_name else "classic"
        e["grouping"] = int(by_name.group(1)) if by_name else 0
        out.append(e)
    # every constant of the type is an entry (a constant this pattern does not take must not pass unseen)
    declared = len(re.findall(r"pub const \w+\s*:\s*CompressionParameters\s*=", text))
    if declared != len(out):
        raise SystemExit(f"{rel}: {declared} CompressionParameters constants, {len(out)} parsed")
    return out


def build(ref):
    root = os.path.join(ref, PARAMS)
    files = sorted(f for f in glob.glob(os.path.join(root, "**", "*.rs"), recursive=True)
                   if "list_compression" in os.path.relpath(f, root) and "noise_squashing" not in os.path.relpath(f, root))
    sets = []
    for f in files:
        sets += parse_file(f, os.path.relpath(f, ref))
    if not sets:
        raise SystemExit(f"no CompressionParameters constant under {root}")
    return sets


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TFHE_RS_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, PARAMS)):
        raise SystemExit(__doc__)
    sets = build(ref)
    json.dump({"_about": "the reference's CompressionParameters constants; see make_compression_sets.py", "sets": sets},
              open(OUT, "w"), indent=1, sort_keys=True)
    print(f"wrote {OUT}: {len(sets)} sets")
