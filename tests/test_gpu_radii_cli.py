"""`--radii` of hs_motif_both_points and hs_motif_both_points_noLSH on the GPU: the output equals the file assembled
from runs with -T over the centres of each radius class; and the whole chain from motif families to their hits --
the centroids and radii hs_center_distance_sampling writes find every member under its own family."""
import json
import os
import subprocess

import numpy as np
import pytest

from hsearch_amd import synth
from tests.test_host_cli import _bin, _tool
from tests.test_radii_cpu import _families

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"
_RADII = (20.0, 40.0, 40.0, 55.0, 0.0)


def _run(cmd, out):
    r = subprocess.run(cmd + ["-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r


def _write_centres(path, names, rows):
    with open(path, "w") as f:
        for nm, row in zip(names, rows):
            f.write("%s\n%s\n" % (nm, " ".join("%.17g" % v for v in row)))


def _assemble(per_class, names):
    """Hits files of the classes (centre-major lines "<centre> <k-mer> <dist>") -> one file in centre order."""
    by_centre = {}
    for text in per_class:
        for line in text.splitlines():
            by_centre.setdefault(line.split(" ")[0], []).append(line)
    return "".join(ln + "\n" for nm in names for ln in by_centre.get(nm, []))


def _class_runs(tmp_path, base_cmd, names, rows, radii, tag, extra=()):
    """(the --radii run's text, the per-class -T runs' texts, stderr of the --radii run)"""
    cen, rad = str(tmp_path / (tag + "_cen")), str(tmp_path / (tag + "_radii"))
    _write_centres(cen, names, rows)
    order = np.random.default_rng(1).permutation(len(names))    # any order in the radii file
    with open(rad, "w") as f:
        f.write("\n" + "".join("%s\t %r  \n" % (names[i], float(radii[i])) for i in order))
    got, r = _run(base_cmd + ["-c", cen, "--radii", rad] + list(extra), str(tmp_path / (tag + "_out")))
    per_class = []
    for R in sorted(set(radii.tolist())):
        sel = np.nonzero(radii == R)[0]
        sub = str(tmp_path / ("%s_cen_%g" % (tag, R)))
        _write_centres(sub, [names[i] for i in sel], rows[sel])
        text, _ = _run(base_cmd + ["-c", sub, "-T", repr(R)] + list(extra), str(tmp_path / ("%s_out_%g" % (tag, R))))
        if R > 0:
            assert text, R
        per_class.append(text)
    return got, per_class, r


def test_radii_flag_equals_per_radius_runs(tmp_path):
    k, K, L, W, seed = 25, 6, 4, 140.0, 81
    rng = np.random.default_rng(17)
    seqs = ["".join(_LETTERS[i] for i in rng.integers(0, 20, size=n)) for n in (900, 1500, 700)]
    fa = str(tmp_path / "db.fa")
    with open(fa, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">prot%d text\n%s\n" % (i, s))
    windows = [s[j:j + k] for s in seqs for j in range(len(s) - k + 1)]
    codes = np.array([[_LETTERS.index(c) for c in w] for w in windows], dtype=np.uint8)
    dbp = str(tmp_path / "db.points")
    with open(dbp, "w") as f:
        for i, row in enumerate(synth.embed(codes)):
            f.write("p%d\n%s\n" % (i, " ".join("%.17g" % v for v in row)))
    nq = 90
    qcodes = codes[rng.choice(len(codes), nq, replace=False)].copy()
    for row in qcodes:
        for _ in range(int(rng.integers(0, 4))):
            row[rng.integers(0, k)] = rng.integers(0, 20)
    names = ["c%d" % i for i in range(nq)]
    radii = np.array(_RADII)[rng.integers(0, len(_RADII), nq)]
    jittered = synth.embed(qcodes) + rng.normal(0, 0.2, size=(nq, 8 * k))
    lsh = [_bin(), "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "--seed", str(seed)]
    nolsh = [_tool("hs_motif_both_points_noLSH"), "-l", str(k)]
    for tag, cmd, rows, extra in (("pts", lsh + ["-d", dbp], jittered, ()),
                                  ("kmers", lsh + ["-d", dbp], synth.embed(qcodes), ("-M", "3")),
                                  ("fa", lsh + ["-d", fa], synth.embed(qcodes), ()),
                                  ("bf", nolsh + ["-d", dbp], jittered, ())):
        got, per_class, r = _class_runs(tmp_path, cmd, names, rows, radii, tag, extra)
        assert got == _assemble(per_class, names), tag
        assert len(got.splitlines()) >= 40, tag
        assert "ignored" not in r.stderr
    # -T beside --radii: ignored, with a notice; --gpus 1 is the one-GPU run
    cen, rad = str(tmp_path / "pts_cen"), str(tmp_path / "pts_radii")
    plain = open(str(tmp_path / "pts_out")).read()
    for cmd in (lsh + ["-d", dbp, "--gpus", "1"], lsh + ["-d", dbp]):
        text, r = _run(cmd + ["-c", cen, "--radii", rad, "-T", "3"], str(tmp_path / "both"))
        assert text == plain and "-T is ignored" in r.stderr
    # FASTA database, one line per matched window (-B): per window the nearest centre over all classes
    got, per_class, _ = _class_runs(tmp_path, lsh + ["-d", fa], names, synth.embed(qcodes), radii, "fab", ("-B", "1"))
    best = {}
    for text in per_class:
        for line in text.splitlines():
            win, centre, dist = line.split(" ")
            assert win not in best or float(dist) != float(best[win][2]), "a tie the printed lines cannot decide"
            if win not in best or float(dist) < float(best[win][2]):
                best[win] = (win, centre, dist)
    want = sorted(best.values(), key=lambda t: int(t[0].rsplit("*", 1)[1]))
    assert got == "".join(" ".join(t) + "\n" for t in want) and len(want) >= 40


def test_families_to_hits_end_to_end(tmp_path, golden_dir):
    """Motif families -> centroids + radii (hs_center_distance_sampling) -> exhaustive search with --radii over the
    families' members: every member is reported under its own family's centroid."""
    t, fam = _families(tmp_path, golden_dir)
    k, out = t["k"], str(tmp_path / "o_")
    r = subprocess.run([_tool("hs_center_distance_sampling"), "-k", fam, "-l", str(k), "-o", out, "-format", "points"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    members = [(f, m, s) for f, seqs in enumerate(t["families"]) for m, s in enumerate(seqs)]
    dbp = str(tmp_path / "members.points")
    with open(dbp, "w") as f:
        for fi, mi, s in members:
            row = synth.embed(np.array([[_LETTERS.index(c) for c in s]], dtype=np.uint8))[0]
            f.write("f%d_m%d\n%s\n" % (fi, mi, " ".join("%.17g" % v for v in row)))
    cmd = [_tool("hs_motif_both_points_noLSH"), "-d", dbp, "-c", out + "hclust.format.txt", "-l", str(k)]
    text, _ = _run(cmd + ["--radii", out + "hclust.radii.txt"], str(tmp_path / "hits"))
    found = {tuple(line.rsplit(" ", 2)[:2]) for line in text.splitlines()}
    for fi, mi, _ in members:
        assert (t["names"][fi], "f%d_m%d" % (fi, mi)) in found, (fi, mi)
