"""The structural cases of hs_proj.hip that tests/test_gpu_proj.py leaves unlaunched, on random inputs, against the
oracle in every hash mode: k that leaves whole padded MFMA steps (17, 29, 41), that fills a step count exactly (16, 28,
40, 52), k < 4; F = K L with a ragged function tile after the first (33, 35, 65), F = 1, K = 31 and 32 (the per-table
tiling aq_tab filled, and one short of it) at strides that are no multiple of 4; n of 1 and around one point tile.
No cross product: each k, each (K, L) and each n occurs once."""
import numpy as np
import pytest

from hsearch_amd import Engine, synth

pytestmark = pytest.mark.gpu

N = 1000
# (k, K, L, build the index too): every k once, every (K, L) once (then (7, 5) again for the remaining k)
SHAPES = [(1, 1, 1, True), (3, 11, 3, True), (16, 7, 5, True), (17, 13, 5, True), (28, 31, 2, True),
          (29, 32, 2, True), (40, 32, 3, True), (41, 7, 5, False), (52, 7, 5, False), (53, 7, 5, False)]


def _inputs(oracle, k, K, L, n):
    W = 8.0 * k + 20.0
    a, b = synth.make_planes(k, K, L, W, seed=100 + k)
    codes = synth.make_db(n, k, seed=200 + k)
    pts = oracle.embed_codes(codes)
    rng = np.random.default_rng(300 + k)
    m = min(n, 300)
    jit = pts[:m] + rng.normal(0.0, 0.7, size=(m, 8 * k))
    return W, a, b, codes, pts, jit


def _check(eng, oracle, a, b, W, codes, pts, jit):
    n, F = len(codes), a.shape[0] * a.shape[1]
    want = oracle.hash_all(a, b, W, pts)
    seen = {}
    for mode in ("exact", "mfma", "auto"):
        eng.set_hash_mode(mode)
        assert np.array_equal(eng.hash_codes(codes), want), mode
        seen[mode] = (eng.profile()["hash_flagged"], eng.profile()["hash_values"])
        assert np.array_equal(eng.hash_points(pts), want), mode
        assert np.array_equal(eng.hash_points(jit), oracle.hash_all(a, b, W, jit)), mode
    assert seen["exact"] == (0, 0)
    return seen


@pytest.mark.parametrize("k,K,L,build", SHAPES)
def test_shapes_in_every_hash_mode(oracle, tmp_path, k, K, L, build):
    W, a, b, codes, pts, jit = _inputs(oracle, k, K, L, N)
    eng = Engine(k, K, L, W, a, b)
    seen = _check(eng, oracle, a, b, W, codes, pts, jit)
    eng.close()
    if k <= 52:
        assert seen["mfma"][1] == N * K * L                # the MFMA pass produced every value
    else:
        assert seen["mfma"] == (0, 0)                      # k > 52: no MFMA variant, the exact kernel
    if not build:
        return
    # the per-table path (table >= 0, out_stride = K): the index built in both modes, byte for byte
    ix = oracle.Index(a, b, W, pts)
    sizes = ix.table_sizes()
    ix.close()
    saved = {}
    for mode in ("mfma", "exact"):
        e = Engine(k, K, L, W, a, b)
        e.set_hash_mode(mode)
        info = e.index_build(codes)
        prof = e.profile()
        path = tmp_path / (mode + ".idx")
        e.index_save(path)
        e.close()
        saved[mode] = path.read_bytes()
        assert info["n_buckets"] == sizes
        assert prof["hash_values"] == (N * K * L if mode == "mfma" else 0)
    assert saved["mfma"] == saved["exact"]


def test_point_counts_around_a_tile(oracle):
    k, K, L = 25, 7, 5
    W, a, b, codes, pts, jit = _inputs(oracle, k, K, L, 129)
    eng = Engine(k, K, L, W, a, b)
    for n in (1, 31, 32, 33, 129):
        seen = _check(eng, oracle, a, b, W, codes[:n], pts[:n], jit[:n])
        assert seen["mfma"][1] == n * K * L
    eng.close()
