"""Clear model of the radix layer for tests/test_radix_bases.py: digits, operand builders that visit every reachable
input of a lookup table BY CONSTRUCTION, and the bookkeeping that tells, from the clear digits alone, which table inputs
and which carry states a call visited.  Plain Python integers; nothing here reads the library.

The correctness reference of every test stays clear big-integer arithmetic on the decrypted blocks.  The model below is
only the coverage accounting: it restates, from the description of the carry look-ahead (the comment that opens the carry
propagation in tfhe_rs_amd/csrc/integer.hip), which value each result table is indexed with, so that a test can assert
that it reached every entry."""
import itertools

import numpy as np

NONE, PROPAGATED, GENERATED = 0, 1, 2


# ------------------------------------------------------------------------------------------ digits
def digits(v, n, msg):
    return [(int(v) // msg ** j) % msg for j in range(n)]


def value(ds, msg):
    return sum(int(d) * msg ** j for j, d in enumerate(ds))


def all_pairs(msg):
    """(a, b) digit rows of msg * msg blocks whose pairs (a_j, b_j) are every pair once."""
    return [i // msg for i in range(msg * msg)], [i % msg for i in range(msg * msg)]


def de_bruijn_row(msg):
    """msg * msg + 1 digits in which every ordered pair of digits occurs as neighbours (in both reading directions: the
    set of all ordered pairs is its own mirror image)."""
    seq, a = [], [0] * (2 * msg)

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, msg):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    assert len(seq) == msg * msg
    return seq + seq[:1]


# ------------------------------------------------------------------------------------------ ciphertexts
def decrypt_many(p, keys, blocks):
    """Decoded values of an array of big-key LWE blocks [..., k N + 1] (common.decode on every block, vectorised)."""
    blocks = np.asarray(blocks, dtype=np.uint64)
    flat = blocks.reshape(-1, blocks.shape[-1])
    sk = np.flatnonzero(keys.glwe_sk)
    out = np.empty(flat.shape[0], dtype=np.uint64)
    delta = np.uint64(p.delta)
    for at in range(0, flat.shape[0], 4096):
        rows = flat[at:at + 4096]
        phase = rows[:, -1] - rows[:, sk].sum(axis=1, dtype=np.uint64)
        out[at:at + 4096] = ((phase + delta // np.uint64(2)) // delta) % np.uint64(2 * p.plaintext_modulus)
    return out.reshape(blocks.shape[:-1]).astype(np.int64)


def encrypt_rows(p, keys, rows, seed):
    """[integer][block] fresh encryptions of digit rows under the big key.  Above 512 blocks the rows are drawn (seeded)
    from a pool of eight fresh encryptions per digit value: the radix layer does not care where a block came from."""
    from .common import encrypt_big
    rows = np.asarray(rows, dtype=np.int64)
    assert rows.ndim == 2 and rows.min(initial=0) >= 0
    if rows.size <= 512:
        return encrypt_big(p, keys, rows.reshape(-1), seed=seed).reshape(rows.shape[0], rows.shape[1], -1)
    top, reps = int(rows.max()) + 1, 8
    pool = encrypt_big(p, keys, [v for v in range(top) for _ in range(reps)], seed=seed)
    pick = np.random.default_rng(seed).integers(0, reps, size=rows.shape)
    return pool[rows * reps + pick]


# ------------------------------------------------------------------------------------------ set cover
def greedy_cover(candidates, visits, universe):
    """A short sub-list of `candidates` whose visits cover `universe`, and what stayed uncovered."""
    missing, chosen = set(universe), []
    seen = [frozenset(visits(c)) for c in candidates]
    while missing:
        best = max(range(len(candidates)), key=lambda i: len(seen[i] & missing))
        if not seen[best] & missing:
            break
        chosen.append(candidates[best])
        missing -= seen[best]
    return chosen, missing


# ------------------------------------------------------------------------------------------ degrees
def bitop_degree(op, a, b):
    """The largest value `a_value op b_value` can take with a_value <= a and b_value <= b (the reference's
    update_degrees_after_bitand / bitor / bitxor)."""
    hi, lo = max(a, b), min(a, b)
    if op == "and":
        return lo
    return max([hi] + [(hi | j) if op == "or" else (hi ^ j) for j in range(lo + 1)])


def clear_bitop(op, a, b):
    return {"and": a & b, "or": a | b, "xor": a ^ b}[op]


# ------------------------------------------------------------------------------------------ carry propagation
def block_state(s, msg):
    return GENERATED if s >= msg else PROPAGATED if s == msg - 1 else NONE


def carries(sums, msg, cin=0):
    """c[j] = the carry entering block j of blocks holding `sums` (c[len] leaves the integer); cin enters block 0."""
    c = [int(cin)]
    for s in sums:
        c.append(int(s + c[-1] >= msg))
    return c


def _join(first, second):
    """state of two neighbours taken together (first is the less significant)"""
    if second == GENERATED or (second == PROPAGATED and first == GENERATED):
        return GENERATED
    return PROPAGATED if second == first == PROPAGATED else NONE


def overflow_pair(a, b, msg):
    """(overflow if a carry arrives, overflow if none) of an addition whose most significant digits are a and b: the
    carry into the sign bit against the carry out of the block, in clear arithmetic."""
    bits = msg.bit_length() - 1
    low = (1 << (bits - 1)) - 1
    return tuple(int((((a & low) + (b & low) + cin) >> (bits - 1)) != ((a + b + cin) >> bits)) for cin in (1, 0))


def propagation_visits(sums, msg, cin=0, flag=None, last_pair=None):
    """What one carry propagation over block sums `sums` (+ cin on block 0) looks up, as the description of the look-ahead
    has it: the first bootstrap of a block reads its sum (one table for block 0, one for the last block, one per position
    in a group of three for the others); a block's result is read off 4 (sum % msg) + z, where z is the carry itself
    ("bit") for the first block of a group of three and for integers of at most four blocks, and otherwise ("z") the
    state of the blocks before it in its group + the carry into the group; the output carry (flag "carry") is read off
    4 (state of the last block) + z; the signed-overflow flag (flag "overflow") off a bivariate table of the operands'
    last blocks `last_pair`, then off its two answers and the same z."""
    L = len(sums)
    x = [int(s) for s in sums]
    x[0] += int(cin)
    if L == 1:
        return {("sum", "single", x[0])}
    c = carries(x, msg)
    st = [block_state(v, msg) for v in x]
    st[0] = GENERATED if x[0] >= msg else NONE          # nothing can arrive in block 0
    out = {("sum", "first" if j == 0 else "last" if j == L - 1 else j % 3, v) for j, v in enumerate(x)}
    for j in range(L):
        if L <= 4 or j % 3 == 0:
            fam, z = "bit", c[j]
        else:
            g = j - j % 3
            before = st[g] if j % 3 == 1 else _join(st[g], st[g + 1])
            fam, z = "z", before + c[g]
            assert (z >= 2) == bool(c[j])
        out.add(("res", fam, x[j] % msg, z))
        if j == L - 1 and flag == "carry":
            out.add(("out", fam, st[j], z))
        if j == L - 1 and flag == "overflow":
            out.add(("ovf_pair", last_pair[0], last_pair[1]))
            out.add(("ovf", fam, overflow_pair(last_pair[0], last_pair[1], msg), z))
    return out


def propagation_universe(msg, widths, flag=None, first_sums=None, top_sum=None):
    """Every entry of the first-bootstrap and result tables (and of the flag's) that integers of the given widths (> 1)
    can reach: sums up to `top_sum` (2 msg - 2), `first_sums` on block 0 (one more with an input carry)."""
    top_sum = 2 * msg - 2 if top_sum is None else top_sum
    first_sums = range(2 * msg) if first_sums is None else first_sums
    u, fams, last_fams = set(), set(), set()
    for L in widths:
        assert L > 1
        for j in range(1, L):
            fam = "bit" if (L <= 4 or j % 3 == 0) else "z"
            fams.add(fam)
            if j == L - 1:
                last_fams.add(fam)
            u |= {("sum", "last" if j == L - 1 else j % 3, v) for v in range(top_sum + 1)}
    u |= {("sum", "first", v) for v in first_sums}
    u |= {("res", "bit", m, 0) for m in range(msg)}      # block 0
    for fam in fams:
        u |= {("res", fam, m, z) for m in range(msg) for z in range(2 if fam == "bit" else 4)}
    pairs = [(a, b) for a in range(msg) for b in range(msg)]
    for fam in last_fams:
        zs = range(2 if fam == "bit" else 4)
        if flag == "carry":
            u |= {("out", fam, s, z) for s in (NONE, PROPAGATED, GENERATED) for z in zs}
        if flag == "overflow":
            u |= {("ovf", fam, overflow_pair(a, b, msg), z) for a, b in pairs for z in zs}
    if flag == "overflow":
        u |= {("ovf_pair", a, b) for a, b in pairs}
    return u


def state_digits(states, msg, rng):
    """Digit rows (a, b) whose block sums realise `states`: below msg - 1, equal to it, or at least msg; which sum, and
    how it splits into two digits, is drawn from rng."""
    a, b = [], []
    for s in states:
        if s == NONE:
            t = int(rng.integers(0, msg - 1))
        elif s == PROPAGATED:
            t = msg - 1
        else:
            t = int(rng.integers(msg, 2 * msg - 1))
        lo, hi = max(0, t - (msg - 1)), min(t, msg - 1)
        x = int(rng.integers(lo, hi + 1))
        a.append(x)
        b.append(t - x)
    return a, b


def state_sequences(L, limit, rng, neighbours=False):
    """All of {none, propagated, generated}^L when that is at most `limit` sequences, else a seeded sample of `limit`
    which holds all-propagated, all-generated, "generated at block 0, then all propagated" and (neighbours) every
    sequence that differs from all-propagated in exactly one block."""
    if 3 ** L <= limit:
        return [tuple(s) for s in itertools.product((NONE, PROPAGATED, GENERATED), repeat=L)]
    must = [(PROPAGATED,) * L, (GENERATED,) * L, (GENERATED,) + (PROPAGATED,) * (L - 1)]
    if neighbours:
        for j in range(L):
            for s in (NONE, GENERATED):
                must.append((PROPAGATED,) * j + (s,) + (PROPAGATED,) * (L - 1 - j))
    must = list(dict.fromkeys(must))
    assert len(must) <= limit
    seen = set(must)
    while len(seen) < limit:
        seen.add(tuple(int(v) for v in rng.integers(0, 3, size=L)))
    return must + sorted(seen - set(must))


# ------------------------------------------------------------------------------------------ equality
def eq_group_size(msg, carry):
    return (msg * carry - 1) // (msg - 1)


def eq_visits(a, b, msg, G):
    """First round: the pairs; then, level by level, (level, members of the group, how many of them were true)."""
    out = {("pair", x, y) for x, y in zip(a, b)}
    bits, level = [int(x == y) for x, y in zip(a, b)], 1
    while len(bits) > 1:
        groups = [bits[i:i + G] for i in range(0, len(bits), G)]
        out |= {("sum", level, len(g), sum(g)) for g in groups}
        bits, level = [int(sum(g) == len(g)) for g in groups], level + 1
    return out


def eq_universe(L, G, with_pairs_of=None):
    """Every (level, group size, sum) an equality of L blocks has.  A level above the first sees results of whole groups, and a
    partial group of the level below is still ONE result: every sum 0 .. c is reachable at every level."""
    u, n, level = set(), L, 1
    while n > 1:
        sizes = {min(G, n - i) for i in range(0, n, G)}
        u |= {("sum", level, c, s) for c in sizes for s in range(c + 1)}
        n, level = (n + G - 1) // G, level + 1
    if with_pairs_of:
        u |= {("pair", x, y) for x in range(with_pairs_of) for y in range(with_pairs_of)}
    return u
