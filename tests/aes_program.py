"""The scheduled AES program of a scratch (hip_test_aes_program), parsed and run on clear values in NumPy: what
tests/test_aes.py checks the schedule with before any bootstrap runs.  Nothing here knows the cipher: a row is a sum of
scaled sources and a constant, looked up in its table."""
import ctypes as C
import dataclasses

import numpy as np

MAGIC = 0x41455350
WIRES, CALLER_A, CALLER_B, CLEAR = 0, 1, 2, 3
BROADCAST, STATE_LANE = 1, 2
IDENTITY, PERM, COLUMN = 0, 1, 2


@dataclasses.dataclass
class Term:
    base: int
    row0: int
    lane_stride: int
    map: int
    flags: int
    scalar: int


@dataclasses.dataclass
class Row:
    table: int
    constant: int
    terms: list
    dst_row0: int
    dst_lane_stride: int
    dst_in_stride: int
    dst_state_lane: int


@dataclasses.dataclass
class Segment:
    lanes: int
    passes: int
    rounds: list          # [(to_caller, [Row])]

    @property
    def rows_per_input(self):
        return sum(len(rows) for _, rows in self.rounds) * self.lanes * self.passes


@dataclasses.dataclass
class Program:
    msg: int
    carry: int
    inputs: int
    parallelism: int
    key_schedule: bool
    cipher_rounds: int
    tables: np.ndarray    # [table][msg * carry]
    maps: np.ndarray      # [permutation][16]
    wire_rows: int
    x: list
    sb: list
    segments: list


def dump(lib, mem):
    n = int(lib.hip_test_aes_program(mem, None, 0))
    buf = (C.c_uint64 * n)()
    assert int(lib.hip_test_aes_program(mem, buf, n)) == n
    return parse(np.frombuffer(buf, dtype=np.uint64).astype(object).tolist())


def parse(w):
    it = iter(w)
    take = lambda k: [int(next(it)) for _ in range(k)]
    magic, msg, carry, inputs, par, ks, rounds, T, E, M, G, wire_rows = take(12)
    assert magic == MAGIC and E == msg * carry
    x, sb = take(8), take(8)
    tables = np.array(take(T * E), dtype=np.int64).reshape(T, E)
    maps = np.array(take(M * 16), dtype=np.int64).reshape(M, 16)
    segments = []
    for _ in range(G):
        lanes, passes, R = take(3)
        rds = []
        for _ in range(R):
            nrows, to_caller = take(2)
            rows = []
            for _ in range(nrows):
                table, constant, nterms, r0, ls, ins, sl = take(7)
                terms = [Term(*take(6)) for _ in range(nterms)]
                rows.append(Row(table, constant, terms, r0, ls, ins, sl))
            rds.append((to_caller, rows))
        segments.append(Segment(lanes, passes, rds))
    assert next(it, None) is None
    return Program(msg, carry, inputs, par, bool(ks), rounds, tables, maps, wire_rows, x, sb, segments)


def source_lane(prog, term, lane0, l):
    if not term.flags & STATE_LANE:
        return l
    lane, kind, par = lane0 + l, term.map & 3, term.map >> 2
    if kind == PERM:
        return int(prog.maps[par][lane])
    if kind == COLUMN:
        return (lane & ~3) | ((lane + par) & 3)
    return lane


def run_segment(prog, seg, wires, caller_a=None, caller_b=None, clear=None, out=None, passes=None, bounds=None):
    """One run of a segment on clear values.  wires / caller_a / caller_b / out: 1-D integer arrays of row values; clear:
    [input][128].
    bounds: a list -> the arrays hold the LARGEST value of every row instead (1 for a caller's bit or a clear bit), a row's
    result is the largest table entry up to its own largest value, and (row, largest value, noise level) of every row is
    appended: the noise level is the sum of |scalar| over the encrypted sources, which are fresh bootstrap outputs or the
    caller's clean blocks at level 1."""
    N = prog.inputs
    bases = {WIRES: wires, CALLER_A: caller_a, CALLER_B: caller_b}
    space = prog.msg * prog.carry
    for p in range(seg.passes if passes is None else passes):
        lane0 = p * seg.lanes
        for to_caller, rows in seg.rounds:
            results = []
            for row in rows:
                for l in range(seg.lanes):
                    for n in range(N):
                        v = row.constant
                        for t in row.terms:
                            if t.base == CLEAR:
                                v += t.scalar * int(clear[n][t.row0])
                                continue
                            r = t.row0 + source_lane(prog, t, lane0, l) * t.lane_stride + (0 if t.flags & BROADCAST else n)
                            v += t.scalar * int(bases[t.base][r])
                        dst = row.dst_row0 + ((lane0 + l) if row.dst_state_lane else l) * row.dst_lane_stride + n * row.dst_in_stride
                        if bounds is None:
                            results.append((dst, int(prog.tables[row.table][v])))
                        else:
                            bounds.append((row, v, sum(t.scalar for t in row.terms if t.base != CLEAR)))
                            results.append((dst, int(prog.tables[row.table][:min(v, space - 1) + 1].max())))
            target = out if to_caller else wires     # a round reads what earlier rounds wrote, never its own rows
            for dst, value in results:
                target[dst] = value
