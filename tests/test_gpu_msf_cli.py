"""`hs_hclust2 -linkage single -tree 1` on the GPU: <o>hclust.tree.txt holds the single-linkage tree Engine.msf finds
under the same planes -- one line per merge in merge order, the distance printed so that it reads back bit for bit --,
the clusters file is what it is without the flag, and -tree goes with -linkage single only."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests import msf_ref as mr
from tests.test_gpu_clustering import _families
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_host_cli import _tool

pytestmark = pytest.mark.gpu


def test_tree_file_is_the_msf_and_the_clusters_file_is_unchanged(tmp_path):
    k, K, L, W, R, seed = 25, 4, 3, 120.0, 50.0, 19
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 20, 30), synth.make_db(400, k, seed=8)])
    rng.shuffle(codes)
    n = len(codes)
    names = ["kmer%d" % i for i in range(n)]
    fa, out, plain = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt"), str(tmp_path / "plain.txt")
    with open(fa, "w") as f:
        for nm, row in zip(names, codes):
            f.write(">%s\n%s\n" % (nm, "".join(_LETTERS[c] for c in row)))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
           "--seed", str(seed), "-linkage", "single"]
    r = subprocess.run(cmd + ["-o", out, "-tree", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a, b = _planes_of_seed(tmp_path, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    want = eng.msf(R, sqrt_test=True, want_label=True)
    eng.close()
    rows = [ln.split(" ") for ln in open(out + "hclust.tree.txt").read().splitlines()]
    assert all(len(row) == 3 for row in rows) and len(rows) == want["n_tree_edges"] > 300
    ids = {nm: i for i, nm in enumerate(names)}
    got = dict(lo=np.array([ids[row[0]] for row in rows], dtype=np.uint32),
               hi=np.array([ids[row[1]] for row in rows], dtype=np.uint32),
               dist=np.array([float(row[2]) for row in rows], dtype=np.float64))
    assert mr.same_tree(got, want)
    assert "num_of_clusters = %d\n" % want["n_components"] in r.stdout
    # without the flag, with -tree 0 and with the short form: the same clusters file; a tree file only where asked
    r = subprocess.run(cmd + ["-o", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(plain).read() == open(out).read() and not os.path.exists(plain + "hclust.tree.txt")
    zero, short = str(tmp_path / "zero.txt"), str(tmp_path / "short.txt")
    r = subprocess.run(cmd + ["-o", zero, "-tree", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(zero).read() == open(out).read() and not os.path.exists(zero + "hclust.tree.txt")
    r = subprocess.run(cmd + ["-o", short, "-t", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(short).read() == open(out).read()
    assert open(short + "hclust.tree.txt").read() == open(out + "hclust.tree.txt").read()


def test_tree_goes_with_single_linkage_only(tmp_path):
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    with open(fa, "w") as f:
        f.write(">a\n%s\n" % (_LETTERS + "ARNDC"))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", "25", "-K", "4", "-L", "3", "-W", "120", "-T", "50", "-o", out]
    for extra in (["-tree", "1"], ["-linkage", "greedy", "-tree", "1"], ["-linkage", "dbscan", "-minpts", "5", "-tree", "1"],
                  ["-linkage", "single", "-tree", "2"], ["-linkage", "single", "-tree", "yes"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "tree" in r.stderr, extra
        assert not os.path.exists(out) and not os.path.exists(out + "hclust.tree.txt"), extra
