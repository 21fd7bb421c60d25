"""bench.py --dump-outputs on the CPU tier: the headline launch's output ciphertexts, written as float64 .npy files,
give back the u64 words exactly (two 32-bit halves) and the centred torus values; a batch larger than DUMP_ROWS is
sampled by a fixed seed and the files stay under 64 MB.  The kernels run in the host emulation with a toy key."""
import os

import numpy as np

from .common import TOY_2048, make_keys
from .harness import oracle_pbs, use_backend


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dumped_outputs_are_the_last_timed_step_bit_for_bit(tmp_path):
    import bench
    lib = use_backend("emu")
    p, keys = TOY_2048, make_keys(TOY_2048)
    _, _, sh, _, _ = bench.run_in_process(lib, p, keys, [0], 5, 2, 1)
    try:
        bench.dump_outputs(str(tmp_path), sh.outputs())
        ref = oracle_pbs(p, keys, "fft64", sh.cts, sh.lut)
    finally:
        sh.close()
    d = _load(str(tmp_path))
    assert sorted(d) == ["pbs_out_hi32", "pbs_out_lo32", "pbs_out_rows", "pbs_out_torus"]
    assert all(a.dtype == np.float64 for a in d.values())
    assert np.array_equal(d["pbs_out_rows"], np.arange(5))
    words = (d["pbs_out_hi32"].astype(np.uint64) << np.uint64(32)) | d["pbs_out_lo32"].astype(np.uint64)
    assert np.array_equal(words, ref)
    assert np.array_equal(d["pbs_out_torus"], ref.view(np.int64) / 2.0 ** 64)
    assert np.all(np.abs(d["pbs_out_torus"]) <= 0.5)


def test_a_large_batch_is_sampled_by_a_fixed_seed_under_64_mb(tmp_path):
    import bench
    rng = np.random.default_rng(5)
    out = rng.integers(0, 1 << 64, size=(4096, 2049), dtype=np.uint64)   # the headline's shape
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out)
    bench.dump_outputs(str(b), out.copy())
    da, db = _load(str(a)), _load(str(b))
    assert all(np.array_equal(da[k], db[k]) for k in da)
    rows = da["pbs_out_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and len(set(rows.tolist())) == len(rows) and np.all(np.diff(rows) > 0)
    words = (da["pbs_out_hi32"].astype(np.uint64) << np.uint64(32)) | da["pbs_out_lo32"].astype(np.uint64)
    assert np.array_equal(words, out[rows])
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 << 20
