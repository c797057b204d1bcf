"""The FP6 join filter's tables and thresholds (hsearch_amd/csrc/hs_join6_tables.h), on the host: no GPU.

The filter value of a member x and a query c is F = sum_p X^[x_p].X^[c_p] - rho(x) - gamma(c) with e2m3 rows X^, and
the contract is one-sided: d^2 <= R^2 implies F >= 2^-6 (the kernel keeps a pair whose accumulator is not negative).
Everything the kernel adds up is a multiple of 2^-6, so F is computed here in INTEGERS (units of 2^-6: exact), from
the codes, the member records and the C operands the library hands out -- the same routines the kernels call.  The
radius of every pair is its own distance (rounded up by a few ulps): the tightest case of the implication."""
import numpy as np
import pytest

from hsearch_amd import capi, synth


def _e2m3_eighths(code):
    code = np.asarray(code, dtype=np.int64)
    m, e = code & 7, (code >> 3) & 3
    v = np.where(e > 0, (8 + m) << np.maximum(e - 1, 0), m)
    return np.where(code & 32, -v, v)


def _table29():
    rng = np.random.default_rng(2906)
    t = synth.coords()
    extra = rng.normal(0.0, np.abs(t).mean() * 1.3, size=(9, 8))
    extra[0, :4] *= 0.01        # a residue near the origin: its codes are subnormal e2m3 values
    extra[1, 0] = -1.9 * np.abs(t[:, :4]).max()   # the row that sets the scale, negative
    return np.ascontiguousarray(np.concatenate([t, extra]))


TABLES = {"aa20": synth.coords, "t29": _table29}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_residue_pair_is_covered(name):
    t = TABLES[name]()
    A = len(t)
    T = capi.join6_tables(t)
    x = t[:, :4]
    assert T["s"] == 7.5 / np.abs(x).max()
    X = _e2m3_eighths(T["codes"]) / 8.0
    # the codes are the nearest grid values: nothing on the grid is closer
    grid = _e2m3_eighths(np.arange(64)) / 8.0
    best = np.abs(T["s"] * x[:, :, None] - grid[None, None, :]).min(axis=2)
    assert np.array_equal(np.abs(T["s"] * x - X), best)
    E = T["s"] ** 2 * (x @ x.T) - X @ X.T
    e = T["e"]
    slack = e[:, None] + e[None, :] - E
    assert slack.min() >= 0.0, (name, slack.min())
    # minimal: every e[a] is held up by one of its constraints
    assert np.all(slack.min(axis=1) < 1e-9)
    assert np.allclose(T["r"], 0.5 * T["s"] ** 2 * (x * x).sum(axis=1) - e, rtol=0, atol=1e-12)
    # the pair table: 48 bits of two residues
    bits = (T["codes"].astype(np.uint64) << (6 * np.arange(4, dtype=np.uint64))).sum(axis=1)
    for r0, r1 in ((0, 0), (3, 17), (A - 1, 1), (A - 1, A - 1)):
        v = int(T["pair"][r1 << 5 | r0, 0]) | int(T["pair"][r1 << 5 | r0, 1]) << 32
        assert v == int(bits[r0]) | int(bits[r1]) << 24


def _decode_records(rec):
    """-(rho - rho0) in 64ths from the 17 slots of member records, against the query side's constant factors."""
    rec = rec.astype(np.uint64)
    word = [int(r[0]) | int(r[1]) << 32 | int(r[2]) << 64 | int(r[3]) << 96 for r in rec]
    out = []
    for w in word:
        total = 0
        for j in range(17):
            d8 = int(_e2m3_eighths((w >> (24 + 6 * j)) & 63))
            f8 = 60 if j < 15 else 4 if j == 15 else 1     # 7.5, 1/2, 1/8 in eighths
            total += d8 * f8                                   # products of eighths = 64ths
        assert w >> (24 + 6 * 17) == 0
        out.append(total)
    return np.array(out, dtype=np.int64), np.array([w & 0xffffff for w in word], dtype=np.int64)


def _pairs(rng, A, k, n_random):
    x = rng.integers(0, A, size=(n_random, k), dtype=np.uint8)
    c = rng.integers(0, A, size=(n_random, k), dtype=np.uint8)
    xs, cs = [x], [c]
    for m in range(6):            # planted: m substitutions
        base = rng.integers(0, A, size=(400, k), dtype=np.uint8)
        mut = base.copy()
        for row in mut:
            pos = rng.choice(k, size=m, replace=False)
            row[pos] = (row[pos] + rng.integers(1, A, size=m)) % A
        xs.append(base)
        cs.append(mut)
    return np.concatenate(xs), np.concatenate(cs)


@pytest.mark.parametrize("k", [21, 25])
@pytest.mark.parametrize("name", sorted(TABLES))
def test_a_pair_within_the_radius_passes(name, k):
    t = TABLES[name]()
    A = len(t)
    rng = np.random.default_rng(600 + k + A)
    x, c = _pairs(rng, A, k, 100000)
    T = capi.join6_tables(t)
    X8 = _e2m3_eighths(T["codes"])                      # [A][4] eighths
    S64 = (X8 @ X8.T).astype(np.int64)                  # residue pair products in 64ths
    d2 = ((t[x] - t[c]) ** 2).sum(axis=(1, 2))          # all 8 columns
    r2 = d2 * (1.0 + 1e-12) + 1e-300                    # the pair's own distance as the radius, rounded up
    mem = capi.join6_thresholds(t, x, 0.0)
    qry = capi.join6_thresholds(t, c, r2)
    slots, pos24 = _decode_records(mem["rec"][:2000])
    # the records say what rho64 says, and carry position 24's codes when the k-mer has one
    assert np.array_equal(slots, -(mem["rho64"][:2000] - mem["rho0_64"]))
    bits = (T["codes"].astype(np.int64) << (6 * np.arange(4))).sum(axis=1)
    assert np.array_equal(pos24, bits[x[:2000, 24]] if k == 25 else np.zeros(2000, dtype=np.int64))
    # multiples of 2^-6 that a float carries exactly, and rho rounded down with one unit to spare
    assert np.abs(qry["c64"]).max() < 1 << 24 and np.abs(mem["rho64"]).max() < 1 << 24
    rho = T["r"][x].sum(axis=1)
    assert np.all(mem["rho64"] <= np.floor(rho * 64.0) - 1 + 1e-6)
    assert np.all(mem["rho64"] >= np.floor(rho * 64.0) - 2)        # (nothing clamped with these tables)
    F64 = S64[x, c].sum(axis=1) - (mem["rho64"] - mem["rho0_64"]) + qry["c64"]
    assert F64.min() >= 1, (name, k, int(F64.min()))
    # and at ONE radius for everybody, as a search has it: hits pass, and the filter still filters
    R = 40.0
    qry = capi.join6_thresholds(t, c, R * R)
    F64 = S64[x, c].sum(axis=1) - (mem["rho64"] - mem["rho0_64"]) + qry["c64"]
    hit = d2 <= R * R * (1.0 + 1e-12)
    assert hit.sum() > 400 and F64[hit].min() >= 1
    if name == "aa20":
        assert (F64[:100000] >= 0).mean() < 0.02


def test_rho_beyond_its_digits_is_clamped_down():
    """A table whose r spans far more than the 15 coarse digits reach: the record then stands for a LOWER rho (more
    pairs pass), never a higher one, and rho0 sits low enough that no rho lies under the digits' range."""
    t = np.zeros((4, 8))
    t[1, :4] = 10.0
    t[2, :4] = -10.0
    t[3, :4] = [10.0, -10.0, 0.3, 0.0]
    k = 25
    kmers = np.array([[0] * k, [1] * k, [2] * k, [1, 2] * 12 + [3], [0] * 24 + [1]], dtype=np.uint8)
    T = capi.join6_tables(t)
    th = capi.join6_thresholds(t, kmers, 0.0)
    rho = np.floor(T["r"][kmers].sum(axis=1) * 64.0) - 1
    assert np.all(th["rho64"] <= rho)
    assert th["rho64"][0] == rho[0] and th["rho64"][1] < rho[1]
    slots, _ = _decode_records(th["rec"])
    assert np.array_equal(slots, -(th["rho64"] - th["rho0_64"]))
