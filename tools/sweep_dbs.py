"""The databases the clustering sweeps under tools/ measure on, so that they all draw the same ones."""


def planted_families(np, n, k, per_family, seed=17):
    """n // per_family random centres, per_family members each with up to 4 substitutions (what
    tests/test_gpu_clustering.py's _families draws), shuffled: uint8 [n'][k]."""
    rng = np.random.default_rng(seed)
    fams = n // per_family
    rows = np.repeat(rng.integers(0, 20, size=(fams, k), dtype=np.uint8), per_family, axis=0)
    n_sub = rng.integers(0, 5, size=len(rows))
    for t in range(4):  # substitution t + 1 of the rows that have that many
        sel = np.nonzero(n_sub > t)[0]
        rows[sel, rng.integers(0, k, size=len(sel))] = rng.integers(0, 20, size=len(sel), dtype=np.uint8)
    rng.shuffle(rows)
    return rows
