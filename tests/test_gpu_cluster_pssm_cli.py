"""`hs_hclust2 -linkage single|dbscan|density -pssm 1` on the GPU: beside the clusters file the program writes the
clusters' profiles and thresholds as <o>hclust.pssm.txt -- exactly what Engine.cluster_pssm gives, in WritePssmFile's
format -- which hs_motif_both_points --pssm consumes unchanged and with which it reports every member of every cluster
under its cluster's name; the switch changes no byte of the clusters file, combines with -centers 1, and is refused
with the greedy linkage, without its companions' master switch and with any other value."""
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests.test_gpu_clustering import _families
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_gpu_dbscan_cli import _fasta
from tests.test_host_cli import _bin, _tool

pytestmark = pytest.mark.gpu

K_LEN, A = 25, 20


def _read_pssm(path):
    names, t, rows = [], [], []
    for line in open(path).read().splitlines():
        if line.startswith(">"):
            name, thr = line[1:].split(" ")
            names.append(name)
            t.append(float(thr))
        else:
            rows.append([float(v) for v in line.split(" ")])
            assert len(rows[-1]) == A
    return names, np.array(t, dtype=np.float64), np.array(rows, dtype=np.float64).reshape(len(names), K_LEN, A)


def _pssm_text(names, S, t):
    """WritePssmFile's format: ">name threshold", then k lines of 20 numbers, every number as %.17g"""
    out = []
    for nm, Sm, tm in zip(names, S, t):
        out.append(">%s %.17g\n" % (nm, tm))
        out += [" ".join("%.17g" % v for v in row) + "\n" for row in Sm]
    return "".join(out)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cluster_pssm_cli")
    k, K, L, W, R, seed, min_pts, min_size = K_LEN, 4, 3, 120.0, 50.0, 19, 5, 10
    rng = np.random.default_rng(3)
    codes = np.concatenate([_families(rng, k, 20, 30), synth.make_db(400, k, seed=8)])
    rng.shuffle(codes)
    names = ["kmer%d" % i for i in range(len(codes))]
    fa = str(tmp / "kmers.fa")
    _fasta(fa, names, codes)
    cmd = [_tool("hs_hclust2"), "-k", fa, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R),
           "--seed", str(seed)]
    a, b = _planes_of_seed(tmp, k, K, L, W, seed)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    yield dict(tmp=tmp, fa=fa, cmd=cmd, codes=codes, names=names, eng=eng, R=R, min_pts=min_pts, min_size=min_size)
    eng.close()


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("linkage,extra,kwargs", [
    ("dbscan", [], dict()),
    ("dbscan", ["-pssm-weights", "columns", "-pssm-threshold", "rank", "-pssm-pseudo", "0.5"],
     dict(weights="columns", threshold="rank", pseudo=0.5)),
    ("single", ["-pssm-weights", "none"], dict(weights="none")),
    ("density", ["-w", "sites", "-H", "cover", "-u", "2"], dict(pseudo=2.0))])
def test_pssm_switch_writes_what_the_library_predicts(world, linkage, extra, kwargs):
    tmp, eng, names, min_size = world["tmp"], world["eng"], world["names"], world["min_size"]
    tag = "%s_%d" % (linkage, len(extra))
    out, plain = str(tmp / (tag + "_with_")), str(tmp / (tag + "_plain_"))
    cmd = world["cmd"] + ["-linkage", linkage] + ([] if linkage == "single" else ["-minpts", str(world["min_pts"])])
    r = _run(cmd + ["-o", out, "-pssm", "1", "-minsize", str(min_size)] + extra)
    assert r.returncode == 0, r.stderr
    r = _run(cmd + ["-o", plain])
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(plain, "rb").read()          # the clusters file: not a byte changes
    mine = sorted(f for f in os.listdir(str(tmp)) if f.startswith(tag))
    core = [tag + "_with_hclust.core.txt"] if linkage == "density" else []
    assert mine == sorted([tag + "_plain_", tag + "_with_", tag + "_with_hclust.pssm.txt"] + core +
                          ([tag + "_plain_hclust.core.txt"] if core else []))
    label = (eng.components(world["R"])["label"] if linkage == "single" else
             eng.dbscan(world["R"], world["min_pts"])["label"] if linkage == "dbscan" else
             eng.density_tree(world["R"], world["min_pts"])["label"])
    want = eng.cluster_pssm(label, min_size, **kwargs)
    rows = len(want["label"])
    assert rows >= 2
    want_names = ["%s:size%d" % (names[l], s) for l, s in zip(want["label"], want["size"])]
    assert open(out + "hclust.pssm.txt").read() == _pssm_text(want_names, want["S"], want["t"])
    got_names, t, S = _read_pssm(out + "hclust.pssm.txt")                   # ... and it reads back bit for bit
    assert got_names == want_names and np.array_equal(t.view(np.uint64), want["t"].view(np.uint64))
    assert np.array_equal(S.view(np.uint64), want["S"].view(np.uint64))


def test_search_reports_every_member_under_its_clusters_name(world):
    """proteins of exactly k residues, one per k-mer: window i is k-mer i"""
    tmp, eng, names, codes, min_size = world["tmp"], world["eng"], world["names"], world["codes"], world["min_size"]
    out, hits, prot = str(tmp / "both_"), str(tmp / "hits.txt"), str(tmp / "proteins.fa")
    cmd = world["cmd"] + ["-linkage", "dbscan", "-minpts", str(world["min_pts"]), "-minsize", str(min_size)]
    r = _run(cmd + ["-o", out, "-centers", "1", "-pssm", "1"])
    assert r.returncode == 0, r.stderr
    assert sorted(f for f in os.listdir(str(tmp)) if f.startswith("both_")) == [
        "both_", "both_hclust.format.txt", "both_hclust.pssm.txt", "both_hclust.radii.txt"]
    only = str(tmp / "centers_")
    r = _run(cmd + ["-o", only, "-centers", "1"])                            # -centers 1 alone writes what it wrote
    assert r.returncode == 0, r.stderr
    for f in ("", "hclust.format.txt", "hclust.radii.txt"):
        assert open(out + f, "rb").read() == open(only + f, "rb").read(), f
    assert not os.path.exists(only + "hclust.pssm.txt")
    _fasta(prot, ["prot%d" % i for i in range(len(codes))], codes)
    r = _run([_bin(), "-d", prot, "-l", str(K_LEN), "--pssm", out + "hclust.pssm.txt", "-o", hits])
    assert r.returncode == 0, r.stdout + r.stderr
    found = set()
    for line in open(hits).read().splitlines():
        name, window, _ = line.split(" ")
        found.add((name, int(window.rsplit("*", 1)[1])))
    label = eng.dbscan(world["R"], world["min_pts"])["label"]
    prof = eng.cluster_profile(label, min_size)
    assert len(prof["label"]) >= 2
    for lab, size in zip(prof["label"], prof["size"]):
        members = np.nonzero(label == lab)[0]
        assert len(members) == size >= min_size
        for i in members:
            assert ("%s:size%d" % (names[lab], size), int(i)) in found, (lab, i)


def test_refusals(world):
    tmp = world["tmp"]
    sub = tmp / "refused"
    sub.mkdir()
    out = str(sub / "clusters.txt")
    cmd = world["cmd"] + ["-o", out]
    single = ["-linkage", "single"]
    for extra, word in ((["-pssm", "1"], "pssm"), (["-linkage", "greedy", "-pssm", "1"], "pssm"),
                        (single + ["-pssm", "yes"], "pssm"), (single + ["-pssm", "2"], "pssm"),
                        (single + ["-pssm-weights", "sites"], "pssm-weights"),
                        (single + ["-pssm", "0", "-pssm-threshold", "cover"], "pssm-threshold"),
                        (single + ["-centers", "1", "-pssm-pseudo", "1"], "pssm-pseudo"),
                        (single + ["-pssm", "1", "-pssm-weights", "site"], "pssm-weights"),
                        (single + ["-pssm", "1", "-pssm-weights", ""], "pssm-weights"),
                        (single + ["-pssm", "1", "-pssm-threshold", "pvalue"], "pssm-threshold"),
                        (single + ["-pssm", "1", "-pssm-pseudo", "0"], "pssm-pseudo"),
                        (single + ["-pssm", "1", "-pssm-pseudo", "nan"], "pssm-pseudo"),
                        (single + ["-pssm", "1", "-pssm-pseudo", "1x"], "pssm-pseudo"),
                        (single + ["-pssm", "1", "-minsize", "0"], "minsize")):
        r = _run(cmd + extra)
        assert r.returncode == 1 and "ERROR:" in r.stderr and word in r.stderr, (extra, r.stderr)
        assert os.listdir(str(sub)) == [], extra
    # -minsize with neither switch: the text it always had, byte for byte
    r = _run(cmd + single + ["-minsize", "5"])
    assert r.returncode == 1 and r.stderr.endswith("ERROR: -minsize goes with -centers 1 only\n")
    assert os.listdir(str(sub)) == []
