"""`hs_hclust2 -linkage dbscan|single -centers 1` on the GPU: beside the clusters file the program writes the clusters'
centroids as a points file and their covering radii, which hs_motif_both_points_noLSH --radii consumes unchanged and
with which it reports every member of every cluster; the switch is an error with the greedy linkage and changes no
byte of the clusters file."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests import summary_ref as sr
from tests.test_gpu_clustering import _families
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_gpu_dbscan_cli import _fasta
from tests.test_host_cli import _tool

pytestmark = pytest.mark.gpu


def _read_points(path, d):
    lines = open(path).read().splitlines()
    assert len(lines) % 2 == 0
    names = lines[0::2]
    rows = np.array([[float(v) for v in ln.split(" ")] for ln in lines[1::2]], dtype=np.float64).reshape(len(names), d)
    return names, rows


def test_centers_switch_writes_centroids_and_radii_a_search_consumes(tmp_path):
    k, K, L, W, R, seed, min_pts, min_size = 25, 4, 3, 120.0, 50.0, 19, 5, 10
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 20, 30), synth.make_db(400, k, seed=8)])
    rng.shuffle(codes)
    n = len(codes)
    names = ["kmer%d" % i for i in range(n)]
    fa, out, plain = str(tmp_path / "kmers.fa"), str(tmp_path / "with_"), str(tmp_path / "plain_")
    _fasta(fa, names, codes)
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
           "--seed", str(seed), "-linkage", "dbscan", "-minpts", str(min_pts)]
    r = subprocess.run(cmd + ["-o", out, "-centers", "1", "-minsize", str(min_size)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(cmd + ["-o", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # without the switch: the same clusters file, byte for byte, and nothing beside it
    assert open(out).read() == open(plain).read()
    assert sorted(os.listdir(str(tmp_path))) == ["kmers.fa", "plain_", "with_", "with_hclust.format.txt",
                                                 "with_hclust.radii.txt"]
    # the two files parse, and are what the library gives for the labels of the same run
    a, b = _planes_of_seed(tmp_path, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    label = eng.dbscan(R, min_pts)["label"]
    prof = eng.cluster_profile(label, min_size)
    rows = len(prof["label"])
    assert rows >= 2
    cen_names, written = _read_points(out + "hclust.format.txt", 8 * k)
    assert cen_names == ["%s:size%d" % (names[l], s) for l, s in zip(prof["label"], prof["size"])]
    assert np.array_equal(written, np.array([[float("%g" % v) for v in row] for row in prof["centroid"]]))
    rad_lines = [ln.rsplit(" ", 1) for ln in open(out + "hclust.radii.txt").read().splitlines()]
    assert [nm for nm, _ in rad_lines] == cen_names
    radii = np.array([float(v) for _, v in rad_lines])
    want = eng.cluster_radii(label, written, min_size)           # against the centres as written and read back
    eng.close()
    assert np.array_equal(radii, want["radius"])
    sr.assert_same(want, sr.radii(codes, label, min_size, synth.coords(), written))
    assert (want["radius"] != sr.radii(codes, label, min_size, synth.coords(), prof["centroid"])["radius"]).any()
    # the exhaustive search consumes both files unchanged and reports every member under its own cluster
    dbp, hits = str(tmp_path / "db.points"), str(tmp_path / "hits")
    with open(dbp, "w") as f:
        for nm, row in zip(names, synth.embed(codes)):
            f.write("%s\n%s\n" % (nm, " ".join("%.17g" % v for v in row)))
    r = subprocess.run([_tool("hs_motif_both_points_noLSH"), "-d", dbp, "-c", out + "hclust.format.txt", "-l", str(k),
                        "--radii", out + "hclust.radii.txt", "-o", hits], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    found = {tuple(line.rsplit(" ", 2)[:2]) for line in open(hits).read().splitlines()}
    for row, lab in enumerate(prof["label"]):
        members = np.nonzero(label == lab)[0]
        assert len(members) == prof["size"][row] >= min_size
        for i in members:
            assert (cen_names[row], names[i]) in found, (row, i)
    # -linkage single takes the switch too; the default -minsize is 50
    single = str(tmp_path / "single_")
    cmd_single = cmd[:-4] + ["-linkage", "single"]
    r = subprocess.run(cmd_single + ["-o", single, "-C", "1", "-m", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert len(_read_points(single + "hclust.format.txt", 8 * k)[0]) >= 2
    r = subprocess.run(cmd + ["-o", str(tmp_path / "big_"), "-centers", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    n_big = int((np.bincount(label[label != capi.NOISE]) >= 50).sum())
    assert len(open(str(tmp_path / "big_hclust.format.txt")).read().splitlines()) == 2 * n_big
    assert len(open(str(tmp_path / "big_hclust.radii.txt")).read().splitlines()) == n_big <= rows


def test_centers_with_the_greedy_linkage_is_an_error(tmp_path):
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    with open(fa, "w") as f:
        f.write(">a\n%s\n" % (_LETTERS + "ARNDC"))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", "25", "-K", "4", "-L", "3", "-W", "120", "-T", "50", "-o", out]
    for extra, word in ((["-centers", "1"], "centers"), (["-linkage", "greedy", "-centers", "1"], "centers"),
                        (["-linkage", "single", "-centers", "yes"], "centers"),
                        (["-linkage", "single", "-minsize", "5"], "minsize"),
                        (["-linkage", "single", "-centers", "1", "-minsize", "0"], "minsize")):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and word in r.stderr, extra
        assert os.listdir(str(tmp_path)) == ["kmers.fa"], extra
