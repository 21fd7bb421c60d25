"""Radix layer, chained: random operation sequences whose operands are the outputs of earlier operations, and the four
ERC-7984 transfer programs, after the reference's long-run tests (integer/server_key/radix_parallel/tests_long_run and
their GPU twins; names only are taken from them, tests/golden/reference_long_run_ops.json).

A sequence is a seeded shuffle of COPIES copies of the executor table of tests/radix_program_model.py on pools of four
samples.  After every step: (a) the result decrypts to the clear function, (b) a second execution on the same operands
gives the same words, degrees, noise levels and bootstrap count, (c) the operands are unchanged, (d) every decrypted block
(message and carry) is at most the degree reported for it, (e) every noise level is within the bound, (f) the bootstrap
count is what the count formula gives.  After the sequence the census is asserted: every operation ran, consumed a produced
operand, the operations that accept unclean operands consumed one, and a divisor 0, an overshift and a produced cmux
condition occurred.  The committed seeds were searched with a dry run of the same draws (`search_seeds`), then run.

[emu] runs the kernel sources on the host with toy keys, [hip] on the MI355X (classic_4_4 there: PARAM_MESSAGE_2_CARRY_2).  On
the emulation and on PARAM_MESSAGE_2_CARRY_2 a schedule is two cases: the second replays the first half without the checks, then
checks the second half and the census; on the emulation only the first half of a shape's first seed is not marked `slow`.
TFHE_HIP_OPSEQ_SEED / TFHE_HIP_OPSEQ_COPIES: another seed / a longer schedule by hand (the census is then printed, not
asserted)."""
import ctypes as C
import dataclasses
import json
import os
import time

import numpy as np
import pytest

from . import compression_helper as ch
from . import radix_model as rm
from . import radix_program_model as rpm
from .common import C1, C4G4
from .test_radix_bases import BASES, Ctx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reference_long_run_ops.json")
REFERENCE = os.environ.get("TFHE_RS_REFERENCE")

COPIES = int(os.environ.get("TFHE_HIP_OPSEQ_COPIES", "2"))
BY_HAND = os.environ.get("TFHE_HIP_OPSEQ_SEED")
# shape -> (blocks, committed seeds).  8 and 9 bits: the smallest widths at which every operation runs all its stages (two
# levels of the carry look-ahead's groups at 4 blocks, column sums, three / four barrel stages, 8 / 9 division iterations)
SHAPES = {"classic_4_4": (4, (11826, 27124)), "classic_8_8": (3, (5248, 5806)), "multibit_g4_4_4": (4, (39652, 27124))}


def base_of(name):
    """the base of tests/test_radix_bases.py; on the emulation with the smallest polynomial that holds its plaintext space
    (the sets of tests/test_div_rem.py: the emulation runs a fibre per lane)"""
    from .test_div_rem import EMU_SMALL
    return dataclasses.replace(next(b for b in BASES if b.name == name), emu=EMU_SMALL[name])


# ------------------------------------------------------------------------------------------ the operation list
def test_executor_table_and_not_wired_list_are_the_reference_operation_list():
    with open(GOLDEN) as f:
        lists = json.load(f)
    names = rpm.reference_names(lists)
    wired = [r for e in rpm.EXECUTORS.values() for r in e.refs]
    assert len(wired) == len(set(wired)), "two executors stand for one reference name"
    assert len(rpm.NOT_WIRED) == len(set(rpm.NOT_WIRED))
    assert not set(wired) & set(rpm.NOT_WIRED), sorted(set(wired) & set(rpm.NOT_WIRED))
    assert set(wired) | set(rpm.NOT_WIRED) == names, (sorted(names - set(wired) - set(rpm.NOT_WIRED)),
                                                     sorted((set(wired) | set(rpm.NOT_WIRED)) - names))
    assert sorted(n for n, e in rpm.EXECUTORS.items() if not e.refs) == sorted(rpm.PROJECT_ONLY)
    assert sorted(lists["erc7984_programs"]) == sorted(PROGRAMS)


@pytest.mark.skipif(not (REFERENCE and os.path.isdir(REFERENCE)), reason="TFHE_RS_REFERENCE does not point to a tfhe-rs tree")
def test_committed_operation_names_are_the_tree_s():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_reference_long_run_ops", os.path.join(HERE, "golden", "make_reference_long_run_ops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(GOLDEN) as f:
        assert json.load(f) == mod.operation_names(REFERENCE)


def test_clear_model_on_known_values():
    """the clear functions against values worked out by hand (8 bits)"""
    assert rpm.clear_signed_div_rem(0x80, 0xFF, 8) == (0x80, 0)            # MIN / -1 wraps
    assert rpm.clear_signed_div_rem(0xF9, 2, 8) == (0xFD, 0xFF)            # -7 / 2 = -3 rem -1
    assert rpm.clear_signed_div_rem(7, 0xFE, 8) == (0xFD, 1)               # 7 / -2 = -3 rem 1
    assert rpm.clear_signed_div_rem(0xF9, 0, 8) == (1, 0xF9) and rpm.clear_signed_div_rem(7, 0, 8) == (0xFF, 7)
    assert rpm.clear_div_rem(7, 0, 8) == (0xFF, 7) and rpm.clear_div_rem(200, 7, 8) == (28, 4)
    assert rpm.clear_shift(0x81, 1, 8, False, True) == 0xC0 and rpm.clear_shift(0x81, 9, 8, False, True) == 0xFF
    assert rpm.clear_shift(0x41, 200, 8, False, True) == 0 and rpm.clear_shift(0x81, 8, 8, True) == 0
    assert rpm.rotl(0x81, 1, 8) == 0x03 and rpm.rotr(0x81, 1, 8) == 0xC0 and rpm.rotl(0x101, 10, 9) == 0x003
    assert rpm.encrypted_rotation(13, 9) == 4 and rpm.encrypted_rotation(29, 9) == 4 and rpm.encrypted_rotation(13, 8) == 5
    assert rpm.negation_degrees([3, 3, 3], 4) == [4, 3, 3]
    assert [rpm.propagate_pbs(L) for L in (1, 2, 4, 10, 13)] == [1, 5, 11, 29, 39]


# ------------------------------------------------------------------------------------------ key material of the value-preserving operations
def rerand_material(h):
    """fused mode (no keyswitch): the public key is derived from the compute key; the same zeros for both executions"""
    if not hasattr(h, "_rerand"):
        from .test_rerand import rerand_key_and_zeros
        h._rerand = rerand_key_and_zeros(h.c.p, h.c.keys, h.c.igpu, h.c.st, "without_ks", h.L, 0x5EED)
    return h._rerand


def compression_material(h):
    """the compression set of the compute set: the reference's on PARAM_MESSAGE_2_CARRY_2, on the toy compute sets the toy
    set whose noise budget tests/compression_helper.py works out"""
    if not hasattr(h, "_compression"):
        from tfhe_rs_amd import core_crypto_gpu as gpu
        from .test_compression import decompression_key
        c = h.c
        cp = ch.REAL if c.p is C1 else ch.TOY_DEC
        ck = ch.make_compression_keys(cp, c.keys.glwe_sk)
        pksk = gpu.CudaLwePackingKeyswitchKey.from_lwe_packing_keyswitch_key(ck.pksk, c.p.big_n, cp.k, cp.N, cp.ks_base_log,
                                                                              cp.ks_level, c.st)
        comp = c.igpu.CudaCompressionKey(pksk, cp.lwe_per_glwe, cp.storage_log_modulus, c.msg, c.carry)
        _, dec = decompression_key(gpu, c.igpu, c.st, cp, ck, c.p, c.keys.glwe_sk)
        h._compression = (comp, dec)
    return h._compression


HELPERS = {"rerand": rerand_material, "compression": compression_material}


# ------------------------------------------------------------------------------------------ sequences
def sequence_cases():
    out = []
    for kind in ("emu", "hip"):
        for shape, (L, seeds) in SHAPES.items():
            for n, seed in enumerate([int(BY_HAND)] if BY_HAND else seeds):
                # a whole schedule costs 5 to 7 s on PARAM_MESSAGE_2_CARRY_2 and 35 to 60 s on the emulation: two cases, the
                # second replays the first half unchecked and checks the second half and the census.  On the emulation the
                # first half of the first seed stands unmarked (the file's unmarked cases: about a minute, what
                # tests/test_div_rem.py costs); every other part carries the `slow` marker
                split = not BY_HAND and (kind == "emu" or shape == "classic_4_4")
                for part in (("first_half", "second_half") if split else ("whole",)):
                    if kind == "hip":
                        marks = [pytest.mark.gpu]
                    else:
                        marks = [] if BY_HAND or (n == 0 and part == "first_half") else [pytest.mark.slow]
                    out.append(pytest.param(kind, shape, seed, part, id=f"{kind}-{shape}-seed_{seed}" +
                                            ("" if part == "whole" else "-" + part), marks=marks))
    return out


@pytest.mark.parametrize("kind,shape,seed,part", sequence_cases())
def test_random_operation_sequence(kind, shape, seed, part):
    base, L = base_of(shape), SHAPES[shape][0]
    print(f"random_op_sequence_test::seed = {seed} ({kind}, {shape}, {L} blocks, {COPIES} copies, {part})")
    c = Ctx(kind, base)
    h = rpm.Runner(c, base.msg, base.carry, L, seed, COPIES, HELPERS)
    assert int(h.lib().hip_integer_propagate_pbs_count(L)) == rpm.propagate_pbs(L)
    half = len(h.schedule) // 2
    start = time.perf_counter()
    try:
        h.run(check_from=half if part == "second_half" else 0, stop=half if part == "first_half" else None)
    finally:
        print("\n".join(h.log[-12:]))
    if part == "first_half":
        print(f"{kind}-{shape}-seed_{seed}: steps 0 .. {half - 1} checked in {time.perf_counter() - start:.1f} s")
        return
    print(f"{kind}-{shape}-seed_{seed}: {h.census_line()}; {h.bootstraps} bootstraps in the operations that report a count; "
          f"{time.perf_counter() - start:.1f} s")
    gaps = h.census_gaps()
    if BY_HAND or COPIES != 2:
        print("census gaps:", gaps)
    else:
        assert not gaps, gaps


def search_seeds(shape, count=2, start=1, limit=2_000_000):
    """seeds whose dry run (same draws, clear values and predicted degrees only) leaves no census gap; the real run
    asserts the census again"""
    base, L = base_of(shape), SHAPES[shape][0]
    found = []
    for seed in range(start, limit):
        if not rpm.Runner(None, base.msg, base.carry, L, seed, 2).run().census_gaps():
            found.append(seed)
            if len(found) == count:
                break
    return found


# ------------------------------------------------------------------------------------------ ERC-7984
MASK64 = (1 << 64) - 1
# (from, to, amount), drawn once (numpy default_rng(7984)) and ordered: enough funds; not enough funds; to + amount overflows
TRANSFERS_64 = [(9143791090806270006, 8872778730490274981, 26868569396036449),
                (54272445031429264, 10600606028203196546, 3389972574747581758),
                (15169110117310765641, 18299343640975390875, 9268884407699112114)]
TRANSFERS_8 = [(200, 17, 55), (54, 100, 55), (255, 201, 55)]          # the same three branches at 8 bits
BRANCHES = [(True, False), (False, False), (True, True)]              # (from >= amount, to + amount overflows)


class Erc:
    """the operations of the programs as the reference's non-assign default operations: the left operand is duplicated"""

    def __init__(self, c, L):
        self.c, self.L, self.top = c, L, c.msg ** L
        self.trace = []

    def dup(self, ct):
        out = ct.duplicate(self.c.st)
        out._info[0][:], out._info[1][:] = ct._info[0], ct._info[1]
        return out

    def keep(self, name, ct, kind="int"):
        self.trace.append((name, ct, kind))
        return ct

    def overflowing_sub(self, name, a, b):
        x = self.dup(a)
        flag = self.c.sks.unsigned_overflowing_sub_assign(x, b, self.c.st)
        return self.keep(name, x), self.keep(name + " borrow", flag, "bool")

    def overflowing_add(self, name, a, b):
        x = self.dup(a)
        flag = self.c.sks.add_assign(x, b, self.c.st, want_carry_out=True)
        return self.keep(name, x), self.keep(name + " carry", flag, "bool")

    def add(self, name, a, b):
        x = self.dup(a)
        self.c.sks.add_assign(x, b, self.c.st)
        return self.keep(name, x)

    def sub(self, name, a, b):
        x = self.dup(a)
        self.c.sks.sub_assign(x, b, self.c.st)
        return self.keep(name, x)

    def mul(self, name, a, b):
        x = self.dup(a)
        self.c.sks.mul_assign(x, b, self.c.st)
        return self.keep(name, x)

    def ge(self, name, a, b):
        return self.keep(name, self.c.sks.compare(a, b, "ge", self.c.st), "bool")

    def bool_or(self, name, p, q):
        x = self.dup(p)
        self.c.sks.bitop_assign(x, q, "or", self.c.st)
        return self.keep(name, x, "bool")

    def bool_not(self, name, p):
        """1 - p: the levelled NOT at message modulus 2, as the reference's boolean_bitnot"""
        x = self.dup(p)
        s, keep = self.c.sks._streams(self.c.st)
        self.c.igpu._lib().cuda_bitnot_ciphertext_64(s, C.byref(x._ffi()), 2, self.c.msg, self.c.carry)
        return self.keep(name, x, "bool")

    def cmux(self, name, k, t, f):
        return self.keep(name, self.c.sks.if_then_else(k, t, f, self.c.st))

    def as_integer(self, flag):
        """the boolean block as the least significant block of an integer whose other blocks are trivial zeros"""
        igpu, st = self.c.igpu, self.c.st
        w = flag.lwe_dimension + 1
        out = igpu.CudaUnsignedRadixCiphertext(igpu.CudaVec(self.L * w, st), 1, self.L, flag.lwe_dimension)
        igpu._lib().cuda_memcpy_async_gpu_to_gpu(out.d_blocks.ptr, flag.d_blocks.ptr, w * 8, st.ptr[0], st.gpu_indexes[0])
        out._info[0][:], out._info[1][:] = 0, 0
        out._info[0][0], out._info[1][0] = flag._info[0][0], flag._info[1][0]
        return out


def safe(e, src, dst, amount):
    new_from, no_funds = e.overflowing_sub("from - amount", src, amount)
    new_to, no_space = e.overflowing_add("to + amount", dst, amount)
    bad = e.bool_or("something not ok", no_funds, no_space)
    e.cmux("new from", bad, src, new_from)
    e.cmux("new to", bad, dst, new_to)


def whitepaper(e, src, dst, amount):
    ok = e.ge("has enough funds", src, amount)
    e.cmux("new to", ok, e.add("to + amount", dst, amount), dst)
    e.cmux("new from", ok, e.sub("from - amount", src, amount), src)


def no_cmux(e, src, dst, amount):
    ok = e.ge("has enough funds", src, amount)
    moved = e.mul("moved amount", amount, e.as_integer(ok))
    e.add("new to", dst, moved)
    e.sub("new from", src, moved)


def overflow(e, src, dst, amount):
    new_from, no_funds = e.overflowing_sub("from - amount", src, amount)
    e.cmux("new from", no_funds, src, new_from)
    ok = e.bool_not("had enough funds", no_funds)
    moved = e.mul("moved amount", amount, e.as_integer(ok))
    e.add("new to", dst, moved)


PROGRAMS = {"safe": safe, "whitepaper": whitepaper, "no_cmux": no_cmux, "overflow": overflow}


def clear_program(name, src, dst, amount, top):
    """every intermediate and final value of a program in `int` arithmetic modulo `top`, by the names the trace uses"""
    enough, space = src >= amount, dst + amount < top
    v = {"from - amount": (src - amount) % top, "from - amount borrow": int(not enough), "to + amount": (dst + amount) % top,
         "to + amount carry": int(not space), "has enough funds": int(enough), "had enough funds": int(enough),
         "moved amount": amount if enough else 0}
    if name == "safe":
        ok = enough and space
        v.update({"something not ok": int(not ok), "new from": (src - amount) % top if ok else src,
                  "new to": (dst + amount) % top if ok else dst})
    else:
        v.update({"new from": (src - amount) % top if enough else src, "new to": (dst + amount) % top if enough else dst})
    return v


ERC_SETS = {"emu-toy_4_blocks": ("emu", "classic_4_4", None, 4, TRANSFERS_8),
            "hip-message_2_carry_2-32_blocks": ("hip", "classic_4_4", None, 32, TRANSFERS_64),
            "hip-gpu_multi_bit_g4-32_blocks": ("hip", "multibit_g4_4_4", C4G4, 32, TRANSFERS_64)}


@pytest.mark.parametrize("program", list(PROGRAMS))
@pytest.mark.parametrize("where", [pytest.param(k, marks=[pytest.mark.gpu] if v[0] == "hip" else []) for k, v in ERC_SETS.items()])
def test_erc7984_transfer(where, program):
    kind, shape, params, L, transfers = ERC_SETS[where]
    base = base_of(shape)
    if params is not None:
        base = dataclasses.replace(base, hip=params)
    c = Ctx(kind, base)
    top = base.msg ** L
    assert top == (1 << 64 if kind == "hip" else 1 << 8)
    start = time.perf_counter()
    for n, ((src, dst, amount), branch) in enumerate(zip(transfers, BRANCHES)):
        assert (src >= amount, dst + amount >= top) == branch, "the transfer does not take the branch it stands for"
        want = clear_program(program, src, dst, amount, top)
        cts = [c.enc([rm.digits(v, L, base.msg)], 7984 + 10 * n + i) for i, v in enumerate((src, dst, amount))]
        for ct in cts:
            ct._info[1][:] = 1
        inputs = [c.words(ct).copy() for ct in cts]
        traces = []
        for _ in range(2):
            e = Erc(c, L)
            PROGRAMS[program](e, *cts)
            traces.append([(name, c.words(ct).copy(), list(map(int, ct._info[0])), kind_) for name, ct, kind_ in e.trace])
        for (name, words, degrees, kind_), (_, again, degrees_again, _) in zip(*traces):
            what = f"{program}, from={src} to={dst} amount={amount}: {name}"
            assert np.array_equal(words, again), f"{what}: two executions differ word for word"
            assert degrees == degrees_again, what
            blocks = [int(x) for x in rm.decrypt_many(c.p, c.keys, words)[0]]
            assert all(x <= d for x, d in zip(blocks, degrees)), f"{what}: blocks {blocks} above degrees {degrees}"
            got = rm.value(blocks, base.msg) % top
            assert got == want[name], f"{what}: {got}, expected {want[name]}"
            assert kind_ == "int" or (len(blocks) == 1 and blocks[0] in (0, 1)), what
        # which branch was taken, from the decrypted flags
        flags = {name: rm.decrypt_many(c.p, c.keys, words)[0][0] for name, words, _, kind_ in traces[0] if kind_ == "bool"}
        if program == "safe":
            assert (flags["from - amount borrow"], flags["to + amount carry"]) == (int(not branch[0]), int(branch[1]))
        else:
            assert flags.get("has enough funds", 1 - flags.get("from - amount borrow", 0)) == int(branch[0])
        for ct, w in zip(cts, inputs):
            assert np.array_equal(c.words(ct), w), "an input was changed"
    print(f"{where} {program}: 3 transfers, each twice, {time.perf_counter() - start:.2f} s")


if __name__ == "__main__":
    for shape_ in SHAPES:
        print(shape_, search_seeds(shape_))
