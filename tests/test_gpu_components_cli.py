"""`hs_hclust2 -linkage single` on the GPU: the clusters file holds the connected components Engine.components
finds under the same planes -- clusters in ascending smallest member, members in ascending index -- and a linkage
the program does not know ends it with status 1."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests.test_gpu_clustering import _families
from tests.test_host_cli import _bin, _tool, _write_points

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"


def _planes_of_seed(tmp_path, k, K, L, W, seed):
    """The planes --seed draws (hsearch::DrawPlanes), as hs_motif_both_points --planes-out dumps them."""
    db, out, planes = [str(tmp_path / x) for x in ("p_db", "p_out", "p_planes")]
    _write_points(db, synth.embed(synth.make_db(4, k, seed=1)), fmt="%g")
    r = subprocess.run([_bin(), "-d", db, "-c", db, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", "1",
                        "-o", out, "--seed", str(seed), "--planes-out", planes], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(planes, dtype=np.float64)
    return raw[:L * K * 8 * k].reshape(L, K, 8 * k), raw[L * K * 8 * k:].reshape(L, K)


def test_linkage_single_writes_the_components(tmp_path):
    k, K, L, W, R, seed = 25, 4, 3, 120.0, 50.0, 19
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 20, 30), synth.make_db(400, k, seed=8)])
    rng.shuffle(codes)
    n = len(codes)
    names = ["kmer%d" % i for i in range(n)]
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    with open(fa, "w") as f:
        for nm, row in zip(names, codes):
            f.write(">%s\n%s\n" % (nm, "".join(_LETTERS[c] for c in row)))
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
           "--seed", str(seed)]
    r = subprocess.run(cmd + ["-o", out, "-linkage", "single"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a, b = _planes_of_seed(tmp_path, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    got = eng.components(R, sqrt_test=True)
    eng.close()
    label = got["label"]
    lines, cid = [], 0
    for i in range(n):
        if label[i] == i:
            members = np.nonzero(label == i)[0]
            lines.append("#clusterid:%d:size%d" % (cid, len(members)))
            lines.extend(names[j] for j in members)
            cid += 1
    text = open(out).read()
    assert text == "\n".join(lines) + "\n"
    sizes = np.bincount(label, minlength=n)
    assert cid == got["n_components"] and (sizes >= 10).sum() >= 2 and (sizes == 1).sum() >= 1
    assert "num_of_clusters = %d\n" % cid in r.stdout
    # the short form is the same option; greedy is what no flag gives, and it is another clustering
    short = str(tmp_path / "short.txt")
    r = subprocess.run(cmd + ["-o", short, "-M", "single"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(short).read() == text
    plain, greedy = str(tmp_path / "plain.txt"), str(tmp_path / "greedy.txt")
    for path, extra in ((plain, []), (greedy, ["-linkage", "greedy"])):
        r = subprocess.run(cmd + ["-o", path] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    assert open(plain).read() == open(greedy).read() != text


def test_unknown_linkage_is_an_error(tmp_path):
    fa, out = str(tmp_path / "kmers.fa"), str(tmp_path / "clusters.txt")
    with open(fa, "w") as f:
        f.write(">a\n%s\n" % (_LETTERS + "ARNDC"))
    r = subprocess.run([_tool("hs_hclust2"), "-k", fa, "-l", "25", "-K", "4", "-L", "3", "-W", "120", "-T", "50", "-o", out,
                        "-linkage", "complete"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "linkage" in r.stderr
    assert not os.path.exists(out)
