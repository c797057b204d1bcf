"""`hs_motif_both_points --topk N` and `hs_hclust2 -knn N` on the GPU: the search's file holds, per centre, the N best
lines of the plain run's file by (distance, k-mer index) -- points and FASTA databases, with -M and --radii --; the
graph file reads back to Engine.self_knn's rows under the same planes, distances bit for bit, and leaves the clusters
file what it was; and the refusals."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests.test_gpu_clustering import _families
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_host_cli import _bin, _tool

pytestmark = pytest.mark.gpu


def _run(cmd, out):
    r = subprocess.run(cmd + ["-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def _best_lines(text, topk, index_of):
    """Of a hits file (centre-major lines "<centre> <k-mer> <dist>") per centre the first topk lines by (dist, k-mer
    index), and the number of centres whose list is cut.  The file prints six digits: where two of a centre's first
    topk + 1 distances print alike, the file cannot tell their order -- asserted not to happen."""
    by_centre, order = {}, []
    for line in text.splitlines():
        centre, kmer, dist = line.split(" ")
        if centre not in by_centre:
            order.append(centre)
        by_centre.setdefault(centre, []).append((float(dist), index_of(kmer), line))
    out, cut = [], 0
    for centre in order:
        rows = sorted(by_centre[centre])
        head = [r[0] for r in rows[:topk + 1]]
        assert len(set(head)) == len(head), "a tie the printed lines cannot decide"
        out += [r[2] for r in rows[:topk]]
        cut += len(rows) > topk
    return "".join(ln + "\n" for ln in out), cut


def test_topk_flag_keeps_the_best_lines_of_the_plain_run(tmp_path):
    k, K, L, W, R, seed, topk = 25, 4, 3, 120.0, 50.0, 19, 3
    rng = np.random.default_rng(11)
    codes = np.unique(np.concatenate([_families(rng, k, 12, 30), synth.make_db(200, k, seed=8)]), axis=0)
    rng.shuffle(codes)
    n = len(codes)
    dbp, fa = str(tmp_path / "db.points"), str(tmp_path / "db.fa")
    with open(dbp, "w") as f:
        for i, row in enumerate(synth.embed(codes)):
            f.write("p%d\n%s\n" % (i, " ".join("%.17g" % v for v in row)))
    with open(fa, "w") as f:                                       # one window per sequence: window number = index
        for i, row in enumerate(codes):
            f.write(">prot%d\n%s\n" % (i, "".join(_LETTERS[c] for c in row)))
    nq = 40
    rows = synth.embed(codes[rng.choice(n, nq, replace=False)]) + rng.normal(0, 0.2, size=(nq, 8 * k))
    names = ["c%d" % i for i in range(nq)]
    cen, rad = str(tmp_path / "centres"), str(tmp_path / "radii")
    with open(cen, "w") as f:
        for nm, row in zip(names, rows):
            f.write("%s\n%s\n" % (nm, " ".join("%.17g" % v for v in row)))
    radii = np.array((30.0, 50.0, 50.0, 60.0))[rng.integers(0, 4, nq)]
    with open(rad, "w") as f:
        f.write("".join("%s %r\n" % (nm, float(r)) for nm, r in zip(names, radii)))
    base = [_bin(), "-c", cen, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "--seed", str(seed)]
    of_point = lambda name: int(name[1:])
    of_window = lambda name: int(name.rsplit("*", 1)[1])
    cases = {"points": (["-d", dbp, "-T", repr(R)], of_point), "probes": (["-d", dbp, "-T", repr(R), "-M", "3"], of_point),
             "fasta": (["-d", fa, "-T", repr(R)], of_window), "radii": (["-d", dbp, "--radii", rad], of_point),
             "fasta radii": (["-d", fa, "--radii", rad], of_window)}
    for what, (args, index_of) in cases.items():
        tag = what.replace(" ", "_")
        plain = _run(base + args, str(tmp_path / (tag + "_plain")))
        got = _run(base + args + ["--topk", str(topk)], str(tmp_path / (tag + "_topk")))
        want, cut = _best_lines(plain, topk, index_of)
        assert got == want, what
        assert cut >= 10 and len(want.splitlines()) < len(plain.splitlines()), what
    # --gpus 1 beside --topk is the one-GPU run; a topk no list reaches changes only the order of the lines
    args = cases["points"][0]
    assert _run(base + args + ["--topk", str(topk), "--gpus", "1"], str(tmp_path / "g1")) == \
        open(str(tmp_path / "points_topk")).read()
    wide = _run(base + args + ["--topk", "64"], str(tmp_path / "wide"))
    plain = open(str(tmp_path / "points_plain")).read()
    assert sorted(wide.splitlines()) == sorted(plain.splitlines())


def test_knn_file_reads_back_to_self_knn(tmp_path):
    k, K, L, W, R, seed, topk = 25, 4, 3, 120.0, 50.0, 19, 4
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
    a, b = _planes_of_seed(tmp_path, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    want = eng.self_knn(R, topk, sqrt_test=True)
    eng.close()
    assert (want["count"] > topk).sum() > 50 and (want["count"] == 0).any()
    ids = {nm: i for i, nm in enumerate(names)}
    for linkage in (["-linkage", "single"], ["-linkage", "dbscan", "-minpts", "3"]):
        tag = linkage[1]
        plain = _run(cmd + linkage, str(tmp_path / (tag + "_plain.txt")))
        out = str(tmp_path / (tag + ".txt"))
        assert _run(cmd + linkage + ["-knn", str(topk)], out) == plain         # the clusters file is what it was
        assert not os.path.exists(str(tmp_path / (tag + "_plain.txt")) + "hclust.knn.txt")
        lines = open(out + "hclust.knn.txt").read().splitlines()
        assert len(lines) == n
        for i, line in enumerate(lines):
            tok = line.split(" ")
            m = min(topk, int(want["count"][i]))
            assert tok[0] == names[i] and int(tok[1]) == want["count"][i] and len(tok) == 2 + 2 * m, i
            assert [ids[t] for t in tok[2::2]] == want["id"][i, :m].tolist(), i
            dist = np.array([float(t) for t in tok[3::2]], dtype=np.float64)
            assert np.array_equal(dist.view(np.uint64), want["dist"][i, :m].view(np.uint64)), i


def test_refusals(tmp_path):
    out = str(tmp_path / "out.txt")
    search = [_bin(), "-d", str(tmp_path / "none.db"), "-c", str(tmp_path / "none.centers"), "-o", out, "-l", "25",
              "-K", "4", "-L", "3", "-W", "120", "-T", "50", "--topk", "3"]
    r = subprocess.run(search + ["--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr == "ERROR: --topk runs on one GPU: it cannot be combined with --gpus 2\n"
    r = subprocess.run(search + ["--best-per-position", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--topk cannot be combined with --best-per-position 1" in r.stderr
    r = subprocess.run([_tool("hs_hclust2"), "-k", str(tmp_path / "none.fa"), "-l", "25", "-K", "4", "-L", "3", "-W", "120",
                        "-T", "50", "-o", out, "-knn", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "-knn goes with -linkage single, dbscan or density" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + "hclust.knn.txt")
