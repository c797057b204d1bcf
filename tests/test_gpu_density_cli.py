"""`hs_hclust2 -linkage density -minpts M -tree 1` on the GPU: the clusters file, <o>hclust.tree.txt and
<o>hclust.core.txt read back to Engine.density_tree's results under the same planes bit for bit; the files of
-linkage dbscan and -linkage single -tree 1 are, byte for byte, what Engine.dbscan / Engine.msf say they were before
`density` became a value of -linkage; and the errors of the new value."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, capi, synth
from tests.test_gpu_clustering import _families
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_host_cli import _tool

pytestmark = pytest.mark.gpu


def _clusters_text(names, label):
    """The clusters file of hsearch::Dbscan / Components for a label array: clusters in ascending label, members in
    ascending index, then the noise block if there is noise."""
    out, cid = [], 0
    for lab in np.unique(label[label != capi.NOISE]):
        members = np.flatnonzero(label == lab)
        out.append("#clusterid:%d:size%d" % (cid, len(members)))
        out += [names[i] for i in members]
        cid += 1
    noise = np.flatnonzero(label == capi.NOISE)
    if len(noise):
        out.append("#noise:size%d" % len(noise))
        out += [names[i] for i in noise]
    return "".join(ln + "\n" for ln in out), cid


def _tree_text(names, lo, hi, w):
    return "".join("%s %s %.17g\n" % (names[x], names[y], v) for x, y, v in zip(lo.tolist(), hi.tolist(), w.tolist()))


def test_density_files_read_back_and_the_other_linkages_are_unchanged(tmp_path):
    k, K, L, W, R, seed, min_pts = 25, 4, 3, 120.0, 50.0, 19, 3
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 8, 30), synth.make_db(160, k, seed=8)])
    rng.shuffle(codes)
    n = len(codes)
    names = ["kmer%d" % i for i in range(n)]
    fa = str(tmp_path / "kmers.fa")
    with open(fa, "w") as f:
        for nm, row in zip(names, codes):
            f.write(">%s\n%s\n" % (nm, "".join(_LETTERS[c] for c in row)))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
           "--seed", str(seed)]

    def run(out, *extra):
        r = subprocess.run(cmd + ["-o", str(tmp_path / out)] + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return str(tmp_path / out), r.stdout

    out, stdout = run("density.txt", "-linkage", "density", "-minpts", str(min_pts), "-tree", "1")
    a, b = _planes_of_seed(tmp_path, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    want = eng.density_tree(R, min_pts, sqrt_test=True)
    db = eng.dbscan(R, min_pts, sqrt_test=True)
    msf = eng.msf(R, sqrt_test=True, want_label=True)
    eng.close()
    assert want["n_tree_edges"] > 100 and 0 < want["n_core"] < n and want["n_clusters"] >= 2
    # the three files, bit for bit
    text, n_clusters = _clusters_text(names, want["label"])
    assert open(out).read() == text and n_clusters == want["n_clusters"]
    assert "num_of_clusters = %d\n" % want["n_clusters"] in stdout
    ids = {nm: i for i, nm in enumerate(names)}
    rows = [ln.split(" ") for ln in open(out + "hclust.tree.txt").read().splitlines()]
    assert all(len(row) == 3 for row in rows) and len(rows) == want["n_tree_edges"]
    assert np.array_equal(np.array([ids[row[0]] for row in rows], dtype=np.uint32), want["lo"])
    assert np.array_equal(np.array([ids[row[1]] for row in rows], dtype=np.uint32), want["hi"])
    assert np.array_equal(np.array([float(row[2]) for row in rows]).view(np.uint64), want["w"].view(np.uint64))
    rows = [ln.split(" ") for ln in open(out + "hclust.core.txt").read().splitlines()]
    assert [row[0] for row in rows] == names and all(len(row) == 2 for row in rows)
    core = np.array([float(row[1]) for row in rows])
    assert np.array_equal(core.view(np.uint64), want["core"].view(np.uint64)) and np.isinf(core).any()
    assert all(row[1] == "inf" for row, c in zip(rows, core) if np.isinf(c))
    # without -tree: the same clusters and core files, no tree file; -centers 1 works as for dbscan
    plain, _ = run("plain.txt", "-linkage", "density", "-minpts", str(min_pts))
    assert open(plain).read() == text and not os.path.exists(plain + "hclust.tree.txt")
    assert open(plain + "hclust.core.txt").read() == open(out + "hclust.core.txt").read()
    cen, _ = run("cen.txt", "-linkage", "density", "-minpts", str(min_pts), "-centers", "1", "-minsize", "10")
    assert open(cen).read() == text and os.path.getsize(cen + "hclust.radii.txt") > 0
    # the other values of -linkage: byte for byte what Engine.dbscan / Engine.msf give
    dbs, _ = run("dbscan.txt", "-linkage", "dbscan", "-minpts", str(min_pts))
    assert open(dbs).read() == _clusters_text(names, db["label"])[0]
    assert not os.path.exists(dbs + "hclust.core.txt") and not os.path.exists(dbs + "hclust.tree.txt")
    sl, _ = run("single.txt", "-linkage", "single", "-tree", "1")
    assert open(sl).read() == _clusters_text(names, msf["label"])[0]
    assert open(sl + "hclust.tree.txt").read() == _tree_text(names, msf["lo"], msf["hi"], msf["dist"])
    assert not os.path.exists(sl + "hclust.core.txt")


def test_errors_of_the_density_linkage(tmp_path):
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    with open(fa, "w") as f:
        f.write(">a\n%s\n" % (_LETTERS + "ARNDC"))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", "25", "-K", "4", "-L", "3", "-W", "120", "-T", "50", "-o", out]
    for extra, word in ((["-linkage", "density"], "minpts"), (["-linkage", "density", "-minpts", "0"], "minpts"),
                        (["-linkage", "density", "-minpts", "3", "-tree", "2"], "tree"),
                        (["-linkage", "dbscan", "-minpts", "5", "-tree", "1"], "tree"),
                        (["-linkage", "single", "-minpts", "5"], "minpts"), (["-linkage", "dense"], "linkage")):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and word in r.stderr, extra
        assert not os.path.exists(out) and not os.path.exists(out + "hclust.core.txt"), extra
    r = subprocess.run(cmd + ["-linkage", "dbscan", "-minpts", "5", "-tree", "1"], capture_output=True, text=True)
    assert r.stderr == "ERROR: -tree goes with -linkage single only: the tree is the single-linkage tree\n"
