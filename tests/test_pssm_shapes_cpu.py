"""The premises of tests/test_gpu_pssm_shapes.py, proved on the host tables (capi.pssm_tables): no GPU.

The GPU tests hold the device to `pssm_survivors == the count the host tables predict` and, for the probe profiles, to
`survivors == hits`.  Both mean something only if the host tables are right at these shapes and the inputs are no
pass-through: that is what is shown here, for every (k, alphabet) of pssm_cases.SHAPES and for the profile families
embedded across a step boundary."""
import numpy as np
import pytest

import pssm_cases
import pssm_ref
from pssm_cases import ALL64, N, NMS, SHAPES, check_invariant


def test_the_shapes_reach_every_instantiation():
    """MFMA steps 1, 2, 3, 4 (the kernels with resident operands) and more than 4 (the NS = 0 kernel); alphabets that
    are no multiple of 4; k * alphabet on a step boundary and one element past it."""
    got = {min(pssm_cases.steps(k, A), 5) for k, A in SHAPES}
    assert got == {1, 2, 3, 4, 5}
    assert sorted({pssm_cases.steps(k, A) for k, A in SHAPES if pssm_cases.steps(k, A) > 4}) == [5, 6]
    assert {A for _, A in SHAPES if A % 4} >= {2, 3, 5, 11, 19, 29, 31}
    ka = {k * A for k, A in SHAPES}
    assert ka >= {128, 256, 384, 512} and ka >= {129, 385, 513}
    assert any(k > 50 for k, _ in SHAPES) and any(25 < k <= 50 for k, _ in SHAPES)     # three and two packed words


@pytest.mark.parametrize("k,A", SHAPES)
def test_mixed_profiles_at_every_shape(k, A):
    case = pssm_cases.mixed_case(k, A, N)
    for nm in NMS:
        hits, passed, T = check_invariant(case["S"][:nm], case["t"][:nm], case["codes"])
        assert np.array_equal(passed, case["surv"][:nm]) and np.array_equal(T["dead"], case["dead"][:nm])
        print("(%d, %d) nm %d: %d hits, %d survivors of %d" % (k, A, nm, hits.sum(), passed.sum(), nm * N))
        assert hits.sum() >= 2
        assert passed.sum() >= hits.sum()
        if nm >= 17:
            assert passed.sum() < nm * N // 2     # the filter is no pass-through on these inputs
    # one k-mer: every profile's threshold is that k-mer's score, but the dead one's
    one = pssm_cases.mixed_case(k, A, 1)
    hits, passed, T = check_invariant(one["S"], one["t"], one["codes"])
    assert hits.sum() == 64 and T["dead"].sum() == 1


@pytest.mark.parametrize("k,A", SHAPES)
def test_probes_make_the_filter_exact(k, A):
    S, t = pssm_cases.probe_profiles(k, A)
    codes = pssm_cases.probe_codes(k, A)
    assert S.shape == (k * A, k, A) and codes.shape == (N, k)
    T = pssm_cases.predict(S, t, codes)["T"]
    sc = pssm_ref.scores(S, codes)
    hit = sc >= t[:, None]
    # profile e = p * A + a is hit by exactly the k-mers with x_p == a
    onehot = (codes[:, :, None] == np.arange(A)[None, None, :]).reshape(len(codes), k * A).T
    assert np.array_equal(hit, onehot)
    F = pssm_ref.filter_values(T["code"], codes)
    passed = (F >= T["tau"][:, None]) & (T["dead"] == 0)[:, None]
    assert np.array_equal(passed, hit), "probe %d, k-mer %d" % tuple(np.argwhere(passed != hit)[0])
    assert not T["dead"].any() and np.all(np.isfinite(T["tau"]))
    print("(%d, %d): fewest hits of a probe %d" % (k, A, hit.sum(axis=1).min()))
    assert hit.sum(axis=1).min() >= 5


@pytest.mark.parametrize("name", list(pssm_cases.FAMILIES))
def test_embedded_families_invariant(name):
    """The family at positions 11 .. 13 of a 25-mer over 20 residues scores what its k = 3 original scores, bit for
    bit, and the invariant holds for it as it does for the original."""
    S, t = pssm_cases.FAMILIES[name]()
    codes = pssm_cases.embedded_codes()
    Se = pssm_cases.embed(S)
    assert Se.shape == (len(S), 25, 20) and np.count_nonzero(Se) == np.count_nonzero(S)
    assert 11 * 20 < 256 < 13 * 20 + 3      # the embedded elements lie on both sides of the step boundary
    sc, sce = pssm_ref.scores(S, ALL64), pssm_ref.scores(Se, codes)
    assert np.array_equal(sc.view(np.uint64), sce.view(np.uint64))
    hits, passed, T = check_invariant(S, t, ALL64)
    hits_e, passed_e, Te = check_invariant(Se, t, codes)
    assert np.array_equal(hits, hits_e)
