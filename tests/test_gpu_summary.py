"""hs_cluster_profile / hs_cluster_radii on the GPU: the clusters of a label array summarised on the device, against the
plain numpy of tests/summary_ref.py and against hs_cluster_summary_codes -- every comparison exact -- for labels of
every source, a cluster that holds everything (rows of hundreds of chunks), every row batching, device pointers, the
chain cluster -> profile -> radii -> search, and the state of the handle."""
import ctypes as C

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import summary_ref as sr
from tests.test_gpu_components import _SHAPES, _db, chain_case
from tests.test_gpu_dbscan import border_case

pytestmark = pytest.mark.gpu

_SEVERAL = [s for s in _SHAPES if s[0] == 25 and s[4] < 100.0][0]   # several clusters
_CHAINED = [s for s in _SHAPES if s[4] > 100.0][0]                   # everything chains into one


def _engine(shape, options=None):
    k, K, L, W, R = shape
    codes = _db(k, R)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    eng = Engine(k, K, L, W, a, b, options=options)
    eng.index_build(codes)
    return eng, codes


@pytest.fixture(scope="module")
def several():
    """One handle at the shape with several clusters, its codes and the three kinds of labels."""
    k, K, L, W, R = _SEVERAL
    eng, codes = _engine(_SEVERAL)
    a, b = synth.make_planes(k, K, L, W, seed=3)
    labels = dict(dbscan=eng.dbscan(R, 5)["label"], components=eng.components(R)["label"],
                  owner=capi.clustering(k, K, L, W, a, b, codes, R)[1])
    assert (labels["dbscan"] == capi.NOISE).sum() >= 100 and len(np.unique(labels["dbscan"])) >= 3
    assert not np.array_equal(labels["components"], labels["owner"])
    yield eng, codes, labels
    eng.close()


_REF = {}


def _want(codes, label, min_size, key):
    """The numpy reference, once per input; hs_cluster_summary_codes must equal it (tests/test_summary_cpu.py pins
    that without a GPU; here it is the second witness)."""
    if key not in _REF:
        want = sr.summary(codes, label, min_size, synth.coords())
        host = capi.cluster_summary_codes(codes, label, min_size, want_counts=True)
        sr.assert_same(host, want, key)
        _REF[key] = want
    return _REF[key]


@pytest.mark.parametrize("min_size", [1, 2, 25])
@pytest.mark.parametrize("source", ["dbscan", "components", "owner"])
def test_label_sources(several, source, min_size):
    eng, codes, labels = several
    want = _want(codes, labels[source], min_size, (source, min_size))
    got = eng.cluster_summary(labels[source], min_size, want_counts=True)
    sr.assert_same(got, want, (source, min_size))
    assert set(got) == set(want) and len(want["label"]) >= 2
    assert len(want["label"]) <= len(codes) // min_size
    if min_size == 1 and source != "dbscan":
        assert want["size"].sum() == len(codes) and (want["size"] == 1).sum() >= 100


@pytest.mark.parametrize("chunk", [0, 64, 7])
def test_one_cluster_of_everything_in_hundreds_of_chunks(chunk):
    eng, codes = _engine(_CHAINED, dict(summary_chunk=chunk))
    n = len(codes)
    label = eng.components(_CHAINED[4])["label"]
    assert (label == 0).all()
    label = np.full(n, 1234, dtype=np.uint32)               # the same cluster under a value that is nobody's root
    want = _want(codes, label, 1, "chained")
    assert list(want["size"]) == [n] and n % 64 != 0 and n % 7 != 0    # a ragged last chunk
    got = eng.cluster_summary(label, 1, want_counts=True)
    sr.assert_same(got, want, chunk)
    eng.close()


@pytest.mark.parametrize("chunk", [0, 7])
def test_rows_that_straddle_chunks(chunk):
    codes, R, _, _, _ = border_case()
    n, k = codes.shape
    W = 1.0e6
    a = np.random.default_rng(1).standard_normal((1, 1, 8 * k))
    b = np.full((1, 1), W / 2)
    eng = Engine(k, 1, 1, W, a, b, options=dict(summary_chunk=chunk))
    eng.index_build(codes)
    for min_pts, min_size in ((4, 1), (3, 3), (2, 5)):
        label = eng.dbscan(R, min_pts)["label"]
        want = _want(codes, label, min_size, ("border", min_pts, min_size))
        # what the input must be for the test to mean something: a row over several chunks of 7 slots, rows smaller
        # than a chunk next to it (the hand-built groups of border_case: at most ten k-mers), and noise among the labels
        assert want["size"].max() >= 4 * 7 and want["size"].min() <= 10 and len(want["size"]) >= 3
        assert (label == capi.NOISE).any()
        sr.assert_same(eng.cluster_summary(label, min_size, want_counts=True), want, (chunk, min_pts, min_size))
    eng.close()


@pytest.mark.parametrize("options", [dict(summary_rows=3), dict(summary_rows=1), dict(summary_rows=3, summary_chunk=7)])
def test_row_batches_and_null_counts(several, options):
    base, codes, labels = several
    eng, _ = _engine(_SEVERAL, options)
    for source, min_size in (("dbscan", 2), ("components", 1)):
        want = _want(codes, labels[source], min_size, (source, min_size))
        with_counts = eng.cluster_profile(labels[source], min_size, want_counts=True)
        without = eng.cluster_profile(labels[source], min_size)
        sr.assert_same(with_counts, want, options)
        sr.assert_same(without, want, options)
        assert "counts" in with_counts and "counts" not in without
        sr.assert_same(base.cluster_profile(labels[source], min_size), want, "default")
    eng.close()


def test_radii_against_other_centres(several):
    eng, codes, labels = several
    label = labels["dbscan"]
    own = _want(codes, label, 2, ("dbscan", 2))
    medoids = synth.embed(codes[own["medoid"]])
    rounded = np.array([[float("%.6g" % v) for v in row] for row in own["centroid"]])
    assert (rounded != own["centroid"]).any()
    for what, centres in (("medoids", medoids), ("rounded", rounded)):
        want = sr.radii(codes, label, 2, synth.coords(), centres)
        sr.assert_same(eng.cluster_radii(label, centres, 2), want, what)
        sr.assert_same(capi.cluster_summary_codes(codes, label, 2, centers=centres), want, what)
        assert (want["max_d2"] != own["max_d2"]).any()


def test_device_forms_and_an_invalid_label_found_on_the_device(several):
    import torch
    eng, codes, labels = several
    n, k = codes.shape
    label = labels["dbscan"]
    want = _want(codes, label, 2, ("dbscan", 2))
    rows = len(want["label"])
    dev = "cuda"
    d_label = torch.from_numpy(label.view(np.int32)).to(dev)
    cap = n // 2

    def poisoned():
        return (torch.full((cap,), 0x7ffffffe, dtype=torch.int32, device=dev),
                torch.full((cap,), 0x7ffffffe, dtype=torch.int32, device=dev),
                torch.full((cap, k, 20), 0x7ffffffe, dtype=torch.int32, device=dev),
                torch.full((cap, 8 * k), -7.5, dtype=torch.float64, device=dev))
    ol, osz, cnt, cen = poisoned()
    torch.cuda.synchronize()
    got_rows = eng.cluster_profile_dev(d_label.data_ptr(), 2, ol.data_ptr(), osz.data_ptr(), cnt.data_ptr(),
                                       cen.data_ptr(), cap)
    assert got_rows == rows
    got = dict(label=ol[:rows].cpu().numpy().view(np.uint32), size=osz[:rows].cpu().numpy().view(np.uint32),
               counts=cnt[:rows].cpu().numpy().view(np.uint32), centroid=cen[:rows].cpu().numpy())
    sr.assert_same(got, want)
    assert (ol[rows:] == 0x7ffffffe).all() and (cen[rows:] == -7.5).all()       # nothing behind the rows
    mx = torch.full((rows,), -7.5, dtype=torch.float64, device=dev)
    rad = torch.full((rows,), -7.5, dtype=torch.float64, device=dev)
    med = torch.full((rows,), 0x7ffffffe, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.cluster_radii_dev(d_label.data_ptr(), 2, cen.data_ptr(), rows, mx.data_ptr(), rad.data_ptr(), med.data_ptr())
    sr.assert_same(dict(max_d2=mx.cpu().numpy(), radius=rad.cpu().numpy(), medoid=med.cpu().numpy().view(np.uint32)),
                   want)
    # without counts, and too small a capacity: the count comes back and nothing is written
    ol2, osz2, _, cen2 = poisoned()
    torch.cuda.synchronize()
    assert eng.cluster_profile_dev(d_label.data_ptr(), 2, ol2.data_ptr(), osz2.data_ptr(), None, cen2.data_ptr(),
                                   cap) == rows
    assert torch.equal(cen2[:rows], cen[:rows]) and torch.equal(ol2[:rows], ol[:rows])
    ol3, osz3, cnt3, cen3 = poisoned()
    torch.cuda.synchronize()
    with pytest.raises(capi.HsError) as e:
        eng.cluster_profile_dev(d_label.data_ptr(), 2, ol3.data_ptr(), osz3.data_ptr(), cnt3.data_ptr(),
                                cen3.data_ptr(), rows - 1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == rows
    # a label that is neither HS_NOISE nor < n, in the last k-mer: found on the device, every output still poisoned
    bad = label.copy()
    bad[n - 1] = n
    d_bad = torch.from_numpy(bad.view(np.int32)).to(dev)
    mx3 = torch.full((rows,), -7.5, dtype=torch.float64, device=dev)
    rad3 = torch.full((rows,), -7.5, dtype=torch.float64, device=dev)
    med3 = torch.full((rows,), 0x7ffffffe, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(capi.HsError) as e:
        eng.cluster_profile_dev(d_bad.data_ptr(), 2, ol3.data_ptr(), osz3.data_ptr(), cnt3.data_ptr(), cen3.data_ptr(),
                                cap)
    assert e.value.status == capi.HS_ERR_INVALID
    with pytest.raises(capi.HsError) as e:
        eng.cluster_radii_dev(d_bad.data_ptr(), 2, cen.data_ptr(), rows, mx3.data_ptr(), rad3.data_ptr(),
                              med3.data_ptr())
    assert e.value.status == capi.HS_ERR_INVALID
    for t in (ol3, osz3, cnt3, med3):
        assert (t == 0x7ffffffe).all()
    for t in (cen3, mx3, rad3):
        assert (t == -7.5).all()
    for call in (lambda: eng.cluster_profile(bad, 2), lambda: eng.cluster_radii(bad, want["centroid"], 2)):
        with pytest.raises(capi.HsError) as e:
            call()
        assert e.value.status == capi.HS_ERR_INVALID


def test_cluster_then_search_with_what_was_found(several, oracle):
    """dbscan_dev -> cluster_profile_dev -> cluster_radii_dev, labels and centroids never leaving the device; then
    a search with the centroids at their radii finds every member of every row under its own row."""
    import torch
    eng, codes, _ = several
    k, K, L, W, R = _SEVERAL
    n = len(codes)
    dev = "cuda"
    min_size = 5
    d_label = torch.empty(n, dtype=torch.int32, device=dev)
    cap = n // min_size
    ol = torch.empty(cap, dtype=torch.int32, device=dev)
    osz = torch.empty(cap, dtype=torch.int32, device=dev)
    cen = torch.empty((cap, 8 * k), dtype=torch.float64, device=dev)
    mx = torch.empty(cap, dtype=torch.float64, device=dev)
    rad = torch.empty(cap, dtype=torch.float64, device=dev)
    med = torch.empty(cap, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.dbscan_dev(d_label.data_ptr(), R, 5)
    rows = eng.cluster_profile_dev(d_label.data_ptr(), min_size, ol.data_ptr(), osz.data_ptr(), None, cen.data_ptr(), cap)
    eng.cluster_radii_dev(d_label.data_ptr(), min_size, cen.data_ptr(), rows, mx.data_ptr(), rad.data_ptr(),
                          med.data_ptr())
    assert rows >= 2
    label = d_label.cpu().numpy().view(np.uint32)
    row_label = ol[:rows].cpu().numpy().view(np.uint32)
    centroids, radii, max_d2 = cen[:rows].cpu().numpy(), rad[:rows].cpu().numpy(), mx[:rows].cpu().numpy()
    hits = eng.bruteforce_radii(centroids, radii)
    d2 = oracle.pairwise_square(oracle.embed_codes(codes), centroids)
    for r in range(rows):
        members = np.nonzero(label == row_label[r])[0]
        assert len(members) == int(osz[r]) >= min_size
        found = hits["id"][hits["q"] == r]
        assert np.isin(members, found).all(), r
        assert d2[r, members].max() == max_d2[r], r                  # the farthest member, to the bit
        assert radii[r] * radii[r] >= max_d2[r] and np.sqrt(max_d2[r]) <= radii[r]
        assert int(med[r]) == members[np.nonzero(d2[r, members] == d2[r, members].min())[0][0]]
    # the LSH search at the same radii reports nothing the brute force does not
    lsh = eng.query_radii(centroids, radii)
    assert np.isin(lsh["q"].astype(np.uint64) << 32 | lsh["id"], hits["q"].astype(np.uint64) << 32 | hits["id"]).all()


def test_no_side_effects_and_errors(several):
    eng, codes, labels = several
    k, K, L, W, R = _SEVERAL
    qcodes = codes[::7].copy()

    def others():
        return (eng.self_join(R), eng.dbscan(R, 5, want_degree=True), eng.query_codes(qcodes, R))
    before = others()
    first = eng.cluster_summary(labels["owner"], 2, want_counts=True)
    eng.cluster_summary(labels["dbscan"], 25)                     # another call in between leaves no trace
    eng.cluster_profile(labels["components"], 1)
    sr.assert_same(eng.cluster_summary(labels["owner"], 2, want_counts=True), first)
    after = others()
    for x, y in zip(before, after):
        assert x.keys() == y.keys()
        for f in x:
            assert np.array_equal(x[f], y[f]), f
    assert len(before[0]["i"]) > 1000 and len(before[2]["q"]) > 1000
    rows = len(first["label"])
    for call in (lambda: eng.cluster_profile(labels["owner"], 0), lambda: eng.cluster_radii(labels["owner"], first["centroid"], 0),
                 lambda: eng.cluster_radii(labels["owner"], first["centroid"][:-1], 2),
                 lambda: eng.cluster_radii(labels["owner"], first["centroid"], 25),
                 lambda: eng.set_option("summary_chunk", -1), lambda: eng.set_option("summary_rows", -1)):
        with pytest.raises(capi.HsError) as e:
            call()
        assert e.value.status == capi.HS_ERR_INVALID
    with pytest.raises(capi.HsError) as e:
        eng.cluster_profile(labels["owner"], 2, cap=rows - 1)
    assert e.value.status == capi.HS_ERR_CAPACITY and e.value.needed == rows
    all_noise = np.full(len(codes), capi.NOISE, dtype=np.uint32)
    none = eng.cluster_summary(all_noise, 1)
    assert all(len(none[f]) == 0 for f in none)
    assert all(len(v) == 0 for v in eng.cluster_summary(labels["owner"], len(codes) + 1).values())
    # an unbuilt index
    a, b = synth.make_planes(k, K, L, W, seed=3)
    fresh = Engine(k, K, L, W, a, b)
    n_out = C.c_uint64(5)
    st = fresh._lib.hs_cluster_profile(fresh._h, capi._vp(all_noise), 1, None, None, None, None, 0, C.byref(n_out))
    assert st == capi.HS_ERR_STATE and n_out.value == 0
    assert fresh._lib.hs_cluster_radii(fresh._h, capi._vp(all_noise), 1, None, 0, None, None, None) == capi.HS_ERR_STATE
    fresh.close()
