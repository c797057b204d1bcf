"""The cluster-summary rule of include/hsearch.h (hs_cluster_profile, hs_cluster_radii) in plain numpy, in exactly the
stated order.  Elementwise numpy products and sums are rounded one by one (no contraction), so this reference is
bit-exact: the centroid loops over the residues a, the d2 over the coordinates t, both vectorised over rows / members."""
import numpy as np

NOISE = 0xffffffff


def rows_of(label, min_size):
    """(the labels of the rows in ascending order, their sizes)"""
    label = np.asarray(label, dtype=np.uint32)
    live = label[label != NOISE]
    vals, sizes = np.unique(live, return_counts=True)
    keep = sizes >= min_size
    return vals[keep].astype(np.uint32), sizes[keep].astype(np.uint32)


def embed(codes, coords):
    return coords[np.asarray(codes)].reshape(len(codes), -1)


def profile(codes, label, min_size, coords):
    codes = np.asarray(codes, dtype=np.uint8)
    label = np.asarray(label, dtype=np.uint32)
    n, k = codes.shape
    alpha = coords.shape[0]
    rl, rs = rows_of(label, min_size)
    m = len(rl)
    counts = np.zeros((m, k, alpha), dtype=np.uint32)
    for r in range(m):
        mem = codes[label == rl[r]]
        for p in range(k):
            counts[r, p] = np.bincount(mem[:, p], minlength=alpha)
    cen = np.zeros((m, k, 8), dtype=np.float64)
    for a in range(alpha):                       # S gains (double)count[p][a] * coords[a][c], a ascending
        prod = counts[:, :, a].astype(np.float64)[:, :, None] * coords[a][None, None, :]
        cen = cen + prod
    cen = cen / rs.astype(np.float64)[:, None, None]
    return dict(label=rl, size=rs, counts=counts, centroid=cen.reshape(m, 8 * k))


def radius_covering(d2):
    r = np.sqrt(d2)
    return np.where(r * r < d2, np.nextafter(r, np.inf), r)


def radii(codes, label, min_size, coords, centers):
    codes = np.asarray(codes, dtype=np.uint8)
    label = np.asarray(label, dtype=np.uint32)
    rl, _ = rows_of(label, min_size)
    m, d = len(rl), 8 * codes.shape[1]
    centers = np.asarray(centers, dtype=np.float64).reshape(m, d)
    max_d2 = np.zeros(m, dtype=np.float64)
    medoid = np.zeros(m, dtype=np.uint32)
    for r in range(m):
        ids = np.nonzero(label == rl[r])[0]
        x = embed(codes[ids], coords)
        d2 = np.zeros(len(ids), dtype=np.float64)
        for t in range(d):                        # left to right
            df = x[:, t] - centers[r, t]
            d2 = d2 + df * df
        max_d2[r] = d2.max()
        medoid[r] = ids[np.nonzero(d2 == d2.min())[0][0]]   # ids ascend: the first at the minimum is the smallest id
    return dict(max_d2=max_d2, radius=radius_covering(max_d2), medoid=medoid)


def summary(codes, label, min_size, coords, centers=None):
    res = profile(codes, label, min_size, coords)
    res.update(radii(codes, label, min_size, coords, res["centroid"] if centers is None else centers))
    return res


def assert_same(got, want, what=""):
    for f in want:
        if f not in got:
            continue
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, f)
        else:
            assert np.array_equal(g, w), (what, f)
