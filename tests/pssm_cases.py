"""Inputs of the PSSM scan's tests, in one place (a helper: nothing here is collected): the (k, alphabet) shapes that
reach every instantiation of the filter kernel and the alphabets whose positions straddle lane chunks and MFMA steps,
the mixed profiles of tests/test_gpu_pssm.py at any profile count, the probe profiles that pin the depth axis element
by element, and the profile families of tests/test_pssm_cpu.py -- as they are (k = 3 over 4 residues) and embedded
across a step boundary of k = 25 over 20 residues.  tests/test_pssm_shapes_cpu.py proves on the host tables what the
GPU tests of tests/test_gpu_pssm_shapes.py take for granted about these inputs."""
import itertools

import numpy as np

from hsearch_amd import capi, synth

try:
    import pssm_ref
except ImportError:
    from tests import pssm_ref

# (k, alphabet) -- k * alphabet, MFMA steps, what it covers.  Steps 1 .. 4 run hs_pssm_filter_kernel<1> .. <4> (NS =
# steps, resident operands), 5 and more the NS = 0 kernel.
SHAPES = [
    (2, 5),     # 10, 1: a small shape
    (8, 16),    # 128, 1: one step, full
    (7, 20),    # 140, 2: position 6 straddles the step boundary
    (43, 3),    # 129, 2: one element in step 2; 11 positions per lane chunk; two packed words
    (64, 4),    # 256, 2: two full steps; three packed words
    (75, 2),    # 150, 2: 16 positions per lane chunk
    (13, 20),   # 260, 3
    (12, 32),   # 384, 3: three full steps
    (35, 11),   # 385, 4: one element in step 4
    (17, 29),   # 493, 4: an odd alphabet
    (16, 32),   # 512, 4: four full steps
    (27, 19),   # 513, 5: NS = 0; one element in step 5
    (21, 31),   # 651, 6: NS = 0; an odd alphabet
]
N = 577        # one full workgroup of 512 members, one full wave and one row
NMS = (1, 17, 65)   # 65: five profile tiles -- one full stage of four with resident operands, then a stage of one

ALL64 = np.array(list(itertools.product(range(4), repeat=3)), dtype=np.uint8)


def steps(k, A):
    return -(-k * A // 128)


def coords(A):
    """Residue coordinates for an alphabet of A = 1 .. 32: the first A rows of synth.coords() up to 20 (None at 20:
    the handle's default), seeded normal rows appended above."""
    assert 1 <= A <= 32
    if A == 20:
        return None
    base = synth.coords()
    if A < 20:
        return np.ascontiguousarray(base[:A])
    rng = np.random.default_rng(77)
    return np.ascontiguousarray(np.concatenate([base, rng.normal(0, 3, size=(A - 20, 8))]))


def engine(k, A, codes=None, hooks=False, options=None):
    from hsearch_amd import Engine
    a, b = synth.make_planes(k, 2, 1, 200.0, seed=3)
    eng = Engine(k, 2, 1, 200.0, a, b, coords=coords(A), hooks=hooks, options=options)
    if codes is not None:
        eng.index_build(codes)
    return eng


def predict(S, t, codes):
    """The host tables of (S, t) and what they let through: dict(T, dead [nm], surv [nm] the k-mers of `codes` that
    pass each profile's filter) -- the count the device's pssm_survivors must equal."""
    T = capi.pssm_tables(S, t)
    F = pssm_ref.filter_values(T["code"], codes)
    surv = ((F >= T["tau"][:, None]) & (T["dead"] == 0)[:, None]).sum(axis=1)
    return dict(T=T, dead=T["dead"], surv=surv)


_MIXED = {}


def mixed_case(k, A, n, nm=65):
    """The recipe of tests/test_gpu_pssm.py::_case at nm profiles: codes [n][k]; entries normal(0, 2), the even
    profiles dyadic (equal scores are common); profile 3 carries a forbidden residue, 5 is dead, 7 passes everything,
    9 has t at its maximum, the others their threshold at the max(1, n // 20)-th best score (attained: the tie is a
    hit).  dict(codes, S, t, sc, T, dead, surv); a prefix of the profiles is a case of its own (the tables are per
    profile).  Computed once per (k, A, n, nm) and never written to."""
    key = (k, A, n, nm)
    if key not in _MIXED:
        rng = np.random.default_rng(1000 * k + 10 * A + n)
        codes = rng.integers(0, A, size=(n, k)).astype(np.uint8)
        S = rng.normal(0, 2, size=(nm, k, A))
        S[::2] = rng.integers(-16, 17, size=S[::2].shape) / 4.0
        if nm > 3:
            S[3, :, 0] = -1e30
        sc = pssm_ref.scores(S, codes)
        t = np.sort(sc, axis=1)[:, -max(1, n // 20)].copy()
        if nm > 5:
            t[5] = sc[5].max() + 1e3
        if nm > 7:
            t[7] = -1e6
        if nm > 9:
            t[9] = sc[9].max()
        case = dict(codes=codes, S=S, t=t, sc=sc, **predict(S, t, codes))
        assert nm <= 7 or (case["dead"][5] == 1 and case["surv"][7] == n)
        for v in (codes, S, t, sc, case["surv"]):
            v.setflags(write=False)
        _MIXED[key] = case
    return _MIXED[key]


def want(case, nm):
    """The contract's result for the first nm profiles of a case: dict(m, id, score, cnt)."""
    hit = case["sc"][:nm] >= case["t"][:nm, None]
    m, i = np.nonzero(hit)
    return dict(m=m.astype(np.uint32), id=i.astype(np.uint32), score=case["sc"][m, i],
                cnt=hit.sum(axis=1).astype(np.uint64))


def probe_profiles(k, A):
    """k * A profiles: profile e has 1.0 at flat element e = p * A + a and 0.0 elsewhere; t = 1 everywhere.  A k-mer
    hits profile e iff x_p == a, and the host tables make the filter exact for these (test_pssm_shapes_cpu.py), so
    every element of the depth axis is tested on its own: an element that either operand puts elsewhere loses hits
    or passes k-mers that are none."""
    return np.eye(k * A).reshape(k * A, k, A), np.ones(k * A)


def probe_codes(k, A, n=N):
    """The k-mers the probes are scanned over: the codes of mixed_case(k, A, n)."""
    return mixed_case(k, A, n)["codes"]


def check_invariant(S, t, codes):
    """Asserts the invariant for profiles S, thresholds t over the k-mers `codes`; returns (hits, passed) [nm]."""
    T = capi.pssm_tables(S, t)
    assert T["code"].max() < 64
    sc = pssm_ref.scores(S, codes)
    hit = sc >= np.asarray(t)[:, None]
    F = pssm_ref.filter_values(T["code"], codes)
    assert np.array_equal(F * 8, np.round(F * 8))
    tau = T["tau"]
    assert np.all((tau * 8 == np.round(tau * 8)) | np.isinf(tau))
    passed = (F >= tau[:, None]) & (T["dead"] == 0)[:, None]
    lost = hit & ~passed
    assert not lost.any(), "profile %d loses k-mer %d" % tuple(np.argwhere(lost)[0])
    assert np.all(np.isposinf(tau) == (T["dead"] == 1))
    return hit.sum(axis=1), passed.sum(axis=1), T


# ---------------------------------------------------------------------------------------------------- the families
# Each returns (S [nm][3][4], t [nm]); tests/test_pssm_cpu.py holds what must be true of them over ALL64.

def random_scales():
    """400 profiles on scales 2^-20 .. 2^20: a forbidden residue beside entries of order 1, constant profiles, dyadic
    ones; thresholds random, equal to an attained score, and at the attainable maximum."""
    rng = np.random.default_rng(2301)
    nm = 400
    scale = 2.0 ** rng.integers(-20, 20, size=(nm, 1, 1))
    S = rng.uniform(-1, 1, size=(nm, 3, 4)) * scale
    S[::7, 1, 2] = -1e30                      # a forbidden residue beside entries of order 1
    S[::11] = S[::11, :1, :1]                 # constant profiles
    S[5::13] = np.round(S[5::13] / scale[5::13] * 4) / 4 * scale[5::13]   # dyadic: many ties
    sc = pssm_ref.scores(S, ALL64)
    t = rng.uniform(-3, 3, size=nm) * scale[:, 0, 0]
    at = rng.integers(0, 64, size=nm)
    t[::3] = sc[np.arange(nm), at][::3]      # thresholds equal to an attained score
    t[1::17] = sc.max(axis=1)[1::17]         # ... the attainable maximum
    return S, t


def outside_profiles():
    """60 profiles on scales 2^-8 .. 2^30, for thresholds outside the range of their scores."""
    rng = np.random.default_rng(2302)
    return rng.normal(size=(60, 3, 4)) * 2.0 ** rng.integers(-8, 30, size=(60, 1, 1))


def threshold_above():
    S = outside_profiles()
    return S, pssm_ref.scores(S, ALL64).max(axis=1) + 1e-3 * np.abs(S).sum(axis=(1, 2))


def threshold_below():
    S = outside_profiles()
    return S, pssm_ref.scores(S, ALL64).min(axis=1) - 1e-3 * np.abs(S).sum(axis=(1, 2))


def threshold_of_any_size(tt):
    """tt: 1e300, -1e300, 1.7e308 or -1.7e308 -- a threshold of any finite size."""
    return outside_profiles(), np.full(60, tt)


def constant_profiles():
    """Zero, 2.5, subnormal entries and the largest legal magnitude, each in every entry."""
    S = np.zeros((4, 3, 4))
    S[1] = 2.5
    S[2] = -1e-310          # subnormal entries
    S[3] = 2.0 ** 100       # the largest legal magnitude
    return S


def constant_at_the_score():
    return constant_profiles(), np.array([0.0, 7.5, -3e-310, 3 * 2.0 ** 100])     # exactly the one attainable score


def constant_below_the_score():
    return constant_profiles(), np.array([-1.0, 7.0, -1.0, 2.0 ** 100])


def constant_above_the_score():
    return constant_profiles(), np.array([1.0, 8.0, 1.0, 2.0 ** 102])


def cancellation():
    """{+-1, +-2^60} in every position order: -1 + 2^60 - 2^60 is 0 in fp64 and -1 over the reals; at t = -0.5 the
    rounded sum is a hit where the real sum is none, and the filter must keep it."""
    big = 2.0 ** 60
    prof, thr = [], []
    for perm in itertools.permutations([1.0, big, big]):
        for half in (1.0, 0.5):
            S = np.array([[v, -v, half * v, -half * v] for v in perm])
            for t in (0.5, -0.5):
                prof.append(S)
                thr.append(t)
    return np.array(prof), np.array(thr)


FAMILIES = {
    "random_scales": random_scales,
    "threshold_above": threshold_above,
    "threshold_below": threshold_below,
    "t=1e300": lambda: threshold_of_any_size(1e300),
    "t=-1e300": lambda: threshold_of_any_size(-1e300),
    "t=1.7e308": lambda: threshold_of_any_size(1.7e308),
    "t=-1.7e308": lambda: threshold_of_any_size(-1.7e308),
    "constant_at_the_score": constant_at_the_score,
    "constant_below_the_score": constant_below_the_score,
    "constant_above_the_score": constant_above_the_score,
    "cancellation": cancellation,
}

# the embedded form: k = 25 over 20 residues; the k = 3 profile sits at positions 11 .. 13, residues 0 .. 3 -- flat
# elements 220 .. 223, 240 .. 243 and 260 .. 263, on both sides of the step boundary at element 256
EMBED_K, EMBED_A, EMBED_P = 25, 20, 11


def embed(S):
    """S [nm][3][4] -> [nm][25][20]: the profile at positions 11 .. 13 and residues 0 .. 3, every other entry 0.0."""
    S = np.asarray(S, dtype=np.float64)
    out = np.zeros((S.shape[0], EMBED_K, EMBED_A))
    out[:, EMBED_P:EMBED_P + 3, :4] = S
    return out


def embedded_codes():
    """64 25-mers whose positions 11 .. 13 run through all 64 triples over residues 0 .. 3 in ALL64's order (k-mer i
    of these scores what 3-mer i of ALL64 scores, bit for bit: the other entries add 0.0); random elsewhere."""
    rng = np.random.default_rng(2305)
    codes = rng.integers(0, EMBED_A, size=(64, EMBED_K)).astype(np.uint8)
    codes[:, EMBED_P:EMBED_P + 3] = ALL64
    return codes
