"""`hs_hclust2 -linkage dbscan -minpts M` on the GPU: the clusters file holds the density clusters Engine.dbscan finds
under the same planes -- clusters in ascending label, members in ascending index, the noise in a last block -- and
-minpts and -linkage dbscan go together or not at all."""
import os
import subprocess

import numpy as np

import pytest

from hsearch_amd import Engine, capi, synth
from tests.test_gpu_clustering import _families
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_host_cli import _tool

pytestmark = pytest.mark.gpu


def _fasta(path, names, codes):
    with open(path, "w") as f:
        for nm, row in zip(names, codes):
            f.write(">%s\n%s\n" % (nm, "".join(_LETTERS[c] for c in row)))


def test_linkage_dbscan_writes_the_density_clusters(tmp_path):
    k, K, L, W, R, seed, min_pts = 25, 4, 3, 120.0, 50.0, 19, 5
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 20, 30), synth.make_db(400, k, seed=8)])
    rng.shuffle(codes)
    n = len(codes)
    names = ["kmer%d" % i for i in range(n)]
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    _fasta(fa, names, codes)
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
           "--seed", str(seed)]
    r = subprocess.run(cmd + ["-o", out, "-linkage", "dbscan", "-minpts", str(min_pts)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    a, b = _planes_of_seed(tmp_path, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    got = eng.dbscan(R, min_pts, sqrt_test=True)
    single = eng.components(R, sqrt_test=True)["label"]
    eng.close()
    label = got["label"]
    lines, cid = [], 0
    for i in range(n):
        members = np.nonzero(label == i)[0]
        if len(members):
            lines.append("#clusterid:%d:size%d" % (cid, len(members)))
            lines.extend(names[j] for j in members)
            cid += 1
    noise = np.nonzero(label == capi.NOISE)[0]
    lines.append("#noise:size%d" % len(noise))
    lines.extend(names[j] for j in noise)
    text = open(out).read()
    assert text == "\n".join(lines) + "\n"
    assert cid == got["n_clusters"] >= 2 and len(noise) == got["n_noise"] >= 100 and got["n_core"] >= 100
    assert "num_of_clusters = %d\n" % cid in r.stdout
    # the short forms are the same options
    short = str(tmp_path / "short.txt")
    r = subprocess.run(cmd + ["-o", short, "-M", "dbscan", "-p", str(min_pts)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(short).read() == text
    # -linkage single is what it was: the components, no noise block
    sing = str(tmp_path / "single.txt")
    r = subprocess.run(cmd + ["-o", sing, "-linkage", "single"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines, cid = [], 0
    for i in range(n):
        if single[i] == i:
            members = np.nonzero(single == i)[0]
            lines.append("#clusterid:%d:size%d" % (cid, len(members)))
            lines.extend(names[j] for j in members)
            cid += 1
    assert open(sing).read() == "\n".join(lines) + "\n" != text
    # min_pts = 1: every k-mer is dense, the clusters are the components and no noise block is written
    one = str(tmp_path / "one.txt")
    r = subprocess.run(cmd + ["-o", one, "-linkage", "dbscan", "-minpts", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(one).read() == open(sing).read()


def test_minpts_and_dbscan_go_together(tmp_path):
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    with open(fa, "w") as f:
        f.write(">a\n%s\n" % (_LETTERS + "ARNDC"))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", "25", "-K", "4", "-L", "3", "-W", "120", "-T", "50", "-o", out]
    for extra in (["-linkage", "dbscan"], ["-minpts", "5"], ["-linkage", "greedy", "-minpts", "5"],
                  ["-linkage", "single", "-minpts", "5"], ["-linkage", "dbscan", "-minpts", "0"],
                  ["-linkage", "dbscan", "-minpts", "few"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "minpts" in r.stderr, extra
        assert not os.path.exists(out), extra
