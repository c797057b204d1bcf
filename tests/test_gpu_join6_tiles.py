"""hs_join6x_kernel's query tiles: the 128-byte rows in the kernel's lane order, the ragged last tile of a segment,
and the threshold C compared outside the MFMA.

The layout (hs_j6_tile_offset, exported as hs_join6_tile_offset) is shared by the gather that writes the tiles and
the kernel that reads them; `test_tile_layout_is_a_bijection` checks it where there is no GPU.

On the GPU the planted case of tests/test_gpu_join8x_issue.py is built the way tests/test_gpu_join6.py builds it,
with other sizes: segments of 128 / 65 / 96 / 97 / 95 queries (last tiles of 32, 1, 32, 1 and 31 rows) against buckets
of 128 / 129 / 127 / 1 / 700 members, a survivor on every member and query slot of the first, pairs exactly on the
radius and one double below in the second.  k = 25 and 21, `join_resident=1` so that every segment takes the
streaming kernel, then the same with items dealt in XCD runs and chunks of 3.  Every result is the oracle's, and
`join_f6_batches` says that the FP6 kernel ran.

Per-query radii: one radius per parity as in test_gpu_join6.test_entry_points (on the FP6 kernel), and queries at
173 -- the largest radius the join takes (R^2 < 30000) -- whichever kernel the plan gives such a call.  Two rules of
the rows cannot be reached through a call and are checked as far as a caller can see them: a NaN radius is refused by hs_query_radii before any row is
made (HS_ERR_INVALID, no hits), and the clamp of C at +2^17 needs R^2 of about 5 * 10^5 with the built-in coordinate
table, where the join is not used; hs_join6_thresholds shows the clamped value on the host."""
import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth

from tests import test_gpu_join8x_issue as planted

SIZES = {"full": (128, 128), "radius": (129, 65), "none": (127, 96), "single": (1, 97), "items": (700, 95)}
R_MAX = 173.0       # R_MAX^2 < 30000: the join still runs
_CASES = {}


def _case(oracle, k):
    """planted._case at k-mer length k with this file's sizes (its module builds one case at a time: set, build,
    restore)."""
    if k not in _CASES:
        keep = planted.K_MER, planted.SIZES
        try:
            planted.K_MER, planted.SIZES = k, SIZES
            planted._CASE.clear()
            _CASES[k] = dict(planted._case(oracle))
        finally:
            planted.K_MER, planted.SIZES = keep
            planted._CASE.clear()
    return _CASES[k]


def _engine(c, k, **opts):
    opts = dict(dict(join_resident=1, join_f6=1), **opts)
    eng = Engine(k, planted.KK, planted.L, planted.W, c["a"], c["b"], options=opts)
    eng.index_build(c["codes"])
    eng.set_verify_mode("join")
    return eng


def test_tile_layout_is_a_bijection():
    """(row, piece) -> byte offset: onto the 16-byte slots of nr * 128 bytes, each once, for every nr; a full tile in
    the kernel's lane order; arguments out of range refused."""
    for nr in range(1, 33):
        off = [capi.join6_tile_offset(nr, j, g) for j in range(nr) for g in range(8)]
        assert sorted(off) == list(range(0, nr * 128, 16)), nr
    for j in range(32):
        c, n = j >> 4, j & 15
        for q in range(4):
            lane = 16 * q + n
            assert capi.join6_tile_offset(32, j, q) == 1024 * (2 * c) + 16 * lane
            assert capi.join6_tile_offset(32, j, 4 + q) == 1024 * (2 * c + 1) + 16 * lane
    for nr in (1, 31):
        for j in range(nr):
            assert [capi.join6_tile_offset(nr, j, g) for g in range(8)] == [16 * (g * nr + j) for g in range(8)]
    for bad in ((0, 0, 0), (33, 0, 0), (5, 5, 0), (32, 0, 8)):
        assert capi.join6_tile_offset(*bad) == 0xffffffff, bad


def test_planted_sizes_hold_on_the_oracle(oracle):
    """No GPU: the construction with this file's sizes (planted._case asserts every planted set on the oracle)."""
    c = _case(oracle, 25)
    assert len(c["want"]["q"]) > 128 and len(c["on_pairs"]) == 2 and len(c["qcodes"]) == 128 + 65 + 96 + 97 + 95


def test_threshold_clamp_on_the_host():
    """C of a query is clamped to +-2^17 (2^23 in 64ths); the radius at which the clamp starts is far beyond the
    join's."""
    t = synth.coords()
    kmers = synth.make_db(8, 25, seed=5)
    big = capi.join6_thresholds(t, kmers, 1e12)["c64"]
    assert (big == 1 << 23).all()
    at_max = capi.join6_thresholds(t, kmers, R_MAX ** 2)["c64"]
    assert (np.abs(at_max) < 1 << 23).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [25, 21])
@pytest.mark.parametrize("routing", ["default", "xcd_runs"])
def test_ragged_and_full_tiles_equal_the_oracle(oracle, k, routing):
    c = _case(oracle, k)
    opts = dict() if routing == "default" else dict(join_xcd_run=2, join_chunk=3)
    eng = _engine(c, k, **opts)
    for R, want in ((c["R"], c["want"]), (c["R_off"], c["want_off"])):
        got = eng.query_codes(c["qcodes"], R)
        p = eng.profile()
        assert p["join_f6_batches"] > 0 and p["join_items_resident"] == 0, p
        planted._assert_equal(got, want, (k, routing, R))
    eng.close()


@pytest.mark.gpu
def test_per_query_radii(oracle):
    k = 25
    c = _case(oracle, k)
    pts, cpts = oracle.embed_codes(c["codes"]), oracle.embed_codes(c["qcodes"])
    nq = len(c["qcodes"])
    ix = oracle.Index(c["a"], c["b"], planted.W, pts)
    want_max = ix.query(cpts, R_MAX)
    ix.close()
    assert len(want_max["q"]) > 10 * len(c["want"]["q"])        # (nearly every in-bucket pair passes at R_MAX)

    def mixed(wants, m):
        """The oracle's answer when query q is searched at the radius of wants[q % m]."""
        parts = [{f: w[f][(w["q"] % m) == r] for f in ("q", "id", "table", "dist")} for r, w in enumerate(wants)]
        order = np.argsort(np.concatenate([p["q"] for p in parts]), kind="stable")
        want = {f: np.concatenate([p[f] for p in parts])[order] for f in ("q", "id", "table", "dist")}
        want["cand"] = c["want"]["cand"]
        return want

    eng = _engine(c, k, wide_rows=2)      # (4-column rows whatever the radius)
    # one radius per parity: even queries at the radius, odd ones a double below -- on the FP6 kernel
    radii = np.where(np.arange(nq) % 2 == 0, c["R"], c["R_off"])
    got = eng.query_radii(c["qcodes"], radii, codes=True)
    assert eng.profile()["join_f6_batches"] > 0
    planted._assert_equal(got, mixed((c["want"], c["want_off"]), 2), "parity radii")
    # a third of the queries at R_MAX, then all of them: the largest C a call can reach (which kernel takes such a
    # call is the plan's business -- the digit bound of the rows from codes may send it to the int8 rows)
    radii = np.choose(np.arange(nq) % 3, [c["R"], c["R_off"], R_MAX])
    got = eng.query_radii(c["qcodes"], radii, codes=True)
    planted._assert_equal(got, mixed((c["want"], c["want_off"], want_max), 3), "radii with R_MAX")
    planted._assert_equal(eng.query_codes(c["qcodes"], R_MAX), want_max, "R_MAX")
    # a NaN radius: refused, no hits
    radii[nq // 2] = np.nan
    with pytest.raises(capi.HsError):
        eng.query_radii(c["qcodes"], radii, codes=True)
    eng.close()
