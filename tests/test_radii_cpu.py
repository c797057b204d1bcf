"""Per-query radii, the parts that need no GPU: the radii file hs_center_distance_sampling -format points writes
(bit for bit the rule of hs_host.hpp FamilyRadii restated in numpy), the `--radii` parser's errors, the refusal of
`--radii` with several GPUs, and the ctypes signatures of the three new entry points."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import hsearch_amd
from hsearch_amd import capi, synth
from tests.onradius_ref import covering_radius
from tests.test_host_cli import _tool


def _families(tmp_path, golden_dir):
    t = json.load(open(os.path.join(golden_dir, "tools.json")))["cluster2datapoint"]
    fam = str(tmp_path / "fams.txt")
    with open(fam, "w") as f:
        for nm, seqs in zip(t["names"], t["families"]):
            f.write(nm + "\n" + "".join(s_ + "\n" for s_ in seqs))
    return t, fam


def parse_radii(path):
    out = {}
    for line in open(path).read().splitlines():
        name, num = line.rsplit(" ", 1)
        assert name not in out
        out[name] = float(num)
    return out


def member_d2(points_text, names, families):
    """d2 of every member to its family's centroid AS PRINTED, summed left to right in fp64."""
    lines = points_text.splitlines()
    assert lines[0::2] == names
    out = []
    for row, seqs in zip(lines[1::2], families):
        c = np.array([float(v) for v in row.split()])
        pts = synth.embed(capi.codes_from_letters(seqs))
        sq = (pts - c[None, :]) ** 2          # each difference and square rounded once
        d2 = np.zeros(len(seqs))
        for i in range(sq.shape[1]):          # left to right
            d2 = d2 + sq[:, i]
        out.append(d2)
    return out


@pytest.mark.parametrize("quantile", [None, "0.5", "1", "0.013"])
def test_radii_file_of_the_family_centroids(tmp_path, golden_dir, quantile):
    t, fam = _families(tmp_path, golden_dir)
    out = str(tmp_path / "o_")
    cmd = [_tool("hs_center_distance_sampling"), "-k", fam, "-l", str(t["k"]), "-o", out, "-format", "points"]
    r = subprocess.run(cmd + (["-q", quantile] if quantile else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(out + "hclust.format.txt").read()
    assert text == t["points_file"]
    got = parse_radii(out + "hclust.radii.txt")
    assert list(got) == t["names"]
    q = float(quantile) if quantile else 1.0
    for name, d2 in zip(t["names"], member_d2(text, t["names"], t["families"])):
        rank = min(max(int(math.ceil(q * len(d2))), 1), len(d2))
        want = covering_radius(float(np.sort(d2)[rank - 1]))
        assert got[name] == want, (name, got[name], want)
        if q == 1.0:   # every member is a hit of its own centroid under the rule d2 <= R * R, and R is tight
            assert (d2 <= got[name] * got[name]).all()
            assert not (d2 <= math.nextafter(got[name], 0.0) ** 2).all()
    # 17 significant digits: the text round-trips
    for line in open(out + "hclust.radii.txt").read().splitlines():
        assert "%.17g" % float(line.rsplit(" ", 1)[1]) == line.rsplit(" ", 1)[1]


def test_radii_file_quantile_is_checked(tmp_path, golden_dir):
    t, fam = _families(tmp_path, golden_dir)
    for bad in ("0", "1.5", "-0.1", "x", "nan"):
        r = subprocess.run([_tool("hs_center_distance_sampling"), "-k", fam, "-l", str(t["k"]), "-o",
                            str(tmp_path / "b_"), "-format", "points", "-q", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "quantile" in r.stderr, bad


def _search_inputs(tmp_path, n_centers=4, k=5):
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 20, size=(30, k), dtype=np.uint8)
    db, cen = str(tmp_path / "db.points"), str(tmp_path / "cen.points")
    with open(db, "w") as f:
        for i, row in enumerate(synth.embed(codes)):
            f.write("p%d\n%s\n" % (i, " ".join("%.17g" % v for v in row)))
    names = ["#PF%05d family %d" % (i, i) for i in range(n_centers)]
    with open(cen, "w") as f:
        for nm, row in zip(names, synth.embed(codes[:n_centers]) + 0.125):
            f.write("%s\n%s\n" % (nm, " ".join("%.17g" % v for v in row)))
    return db, cen, names, k


@pytest.mark.parametrize("prog", ["hs_motif_both_points", "hs_motif_both_points_noLSH"])
def test_radii_file_errors_exit_one_before_any_gpu_work(tmp_path, prog):
    db, cen, names, k = _search_inputs(tmp_path)
    common = [_tool(prog), "-d", db, "-c", cen, "-l", str(k), "-o", str(tmp_path / "out")]
    if prog == "hs_motif_both_points":
        common += ["-W", "50", "--seed", "1"]
    good = ["%s %r" % (nm, 10.0 + i) for i, nm in enumerate(names)]
    cases = {
        "no radius for centre": good[:2] + good[3:],
        "has a radius already": good + [good[1]],
        "is not a centre": good + ["#PF99999 nobody 3.5"],
        "is not a radius": good[:3] + [names[3] + " 12.5x"],
        "is not a radius ": good[:3] + [names[3] + " nan"],
        "expected '<centre name> <radius>'": good[:3] + ["12.5"],
    }
    for what, lines in cases.items():
        path = str(tmp_path / "radii.txt")
        open(path, "w").write("\n".join(lines) + "\n")
        r = subprocess.run(common + ["--radii", path], capture_output=True, text=True)
        assert r.returncode == 1 and what.strip() in r.stderr, (what, r.stderr)
        assert not os.path.exists(str(tmp_path / "out"))
    r = subprocess.run(common + ["--radii", str(tmp_path / "missing.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr
    # neither -T nor --radii: a missing required option, as before
    r = subprocess.run(common, capture_output=True, text=True)
    assert r.returncode == 0 and "missing required option -T" in r.stderr


def test_radii_with_several_gpus_is_refused(tmp_path):
    db, cen, names, k = _search_inputs(tmp_path)
    path = str(tmp_path / "radii.txt")
    open(path, "w").write("".join("%s 10\n" % nm for nm in names))
    r = subprocess.run([_tool("hs_motif_both_points"), "-d", db, "-c", cen, "-l", str(k), "-W", "50", "-o",
                        str(tmp_path / "out"), "--radii", path, "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "--radii" in r.stderr and "--gpus" in r.stderr
    assert not os.path.exists(str(tmp_path / "out"))


def test_new_entry_points_resolve_with_their_signatures():
    lib = hsearch_amd.load()
    vp, u64 = C.c_void_p, C.c_uint64
    query = [vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp]
    assert lib.hs_query_radii.argtypes == query and lib.hs_query_radii_dev.argtypes == query
    assert lib.hs_bruteforce_radii.argtypes == [vp, vp, u64, vp, vp, vp, vp, u64, C.POINTER(u64)]
    for name in ("hs_query_radii", "hs_query_radii_dev", "hs_bruteforce_radii"):
        assert getattr(lib, name).restype == C.c_int and name in capi.EXPORTS
    # no handle: refused before anything else is looked at
    n = u64(7)
    assert lib.hs_query_radii(None, None, None, 0, None, None, None, None, None, 0, C.byref(n), None) == capi.HS_ERR_INVALID
    assert lib.hs_query_radii_dev(None, None, None, 0, None, None, None, None, None, 0, C.byref(n), None) == capi.HS_ERR_INVALID
    assert lib.hs_bruteforce_radii(None, None, 0, None, None, None, None, 0, C.byref(n)) == capi.HS_ERR_INVALID
    for name in ("query_radii", "query_radii_dev", "bruteforce_radii"):
        assert callable(getattr(capi.Engine, name))
