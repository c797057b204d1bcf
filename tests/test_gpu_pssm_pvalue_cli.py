"""`hs_motif_both_points --pssm FILE --pssm-pvalue P --pssm-out FILE2` on the GPU over the planted-family FASTA
database of tests/test_gpu_pssm_refine_cli.py: FILE2 is FILE with every threshold replaced by
Engine.pssm_pvalue_threshold's under the database's residue composition, bit for bit and the matrices untouched; the -o
file is byte for byte what a run with --pssm FILE2 writes (with --pssm-top and --pssm-per-sequence too); the clipped
and the empty profiles are named on stderr; --pssm-pvalue-column appends Engine.pssm_pvalue's p_hi; and the refused
flag combinations."""
import subprocess

import numpy as np
import pytest

from tests.test_gpu_pssm_counts import K
from tests.test_gpu_pssm_refine_cli import _NAMES, _read_pssm, world  # noqa: F401  (world: the module's fixture)
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

P = "1e-4"
FLOOR = "-40"


@pytest.mark.parametrize("mode", ["hits", "per-sequence", "top"])
def test_pvalue_file_and_output(world, mode):
    tmp = world["tmp"]
    out, out2, pf2 = str(tmp / (mode + "_p.txt")), str(tmp / (mode + "_p2.txt")), str(tmp / (mode + "_p.pssm"))
    extra = {"hits": [], "per-sequence": ["--pssm-per-sequence", "1"], "top": ["--pssm-top", "3"]}[mode]
    base = [_bin(), "-d", world["fa"], "-l", str(K)]
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-pvalue", P, "--pssm-null-floor", FLOOR, "--pssm-out", pf2,
                               "-o", out] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = world["eng"].pssm_pvalue_threshold(world["loose"], float(P), t_lo=float(FLOOR))
    names, t, S = _read_pssm(pf2)
    assert names == _NAMES and np.array_equal(t.view(np.uint64), want["t"].view(np.uint64))
    assert np.array_equal(S.view(np.uint64), world["loose"].view(np.uint64))       # the matrices as FILE gives them
    assert not np.array_equal(t, world["t"]) and np.all(want["p_hi"] <= float(P))
    assert _file2_bytes_reproduce(pf2, names, S, t, tmp / (mode + "_again.pssm"))
    r = subprocess.run(base + ["--pssm", pf2, "-o", out2] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(out, "rb").read()
    assert got == open(out2, "rb").read()
    if mode == "hits":
        hits = world["eng"].pssm_scan(world["loose"], want["t"])
        assert len(got.splitlines()) == len(hits["m"]) and "number of hits %d" % len(hits["m"]) in r.stdout


def _file2_bytes_reproduce(pf2, names, S, t, again):
    """FILE2 went through WritePssmFile: every number is %.17g and reads back bit for bit"""
    with open(str(again), "w") as f:
        for nm, prof, thr in zip(names, S, t):
            f.write(">%s %.17g\n" % (nm, thr))
            for row in prof:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    return open(str(again), "rb").read() == open(pf2, "rb").read()


def test_flags_on_stderr(world):
    tmp = world["tmp"]
    out, pf2 = str(tmp / "flags.txt"), str(tmp / "flags.pssm")
    base = [_bin(), "-d", world["fa"], "-l", str(K), "-o", out, "--pssm", world["pf"], "--pssm-out", pf2]
    # nothing is admissible at 1e-300: every profile keeps +DBL_MAX and finds nothing
    r = subprocess.run(base + ["--pssm-pvalue", "1e-300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = world["eng"].pssm_pvalue_threshold(world["loose"], 1e-300)
    assert np.all(want["flag"] == 2) and all("profile %s:" % n in r.stderr and "DBL_MAX" in r.stderr for n in _NAMES)
    names, t, _ = _read_pssm(pf2)
    assert np.all(t == 1.7976931348623157e308) and "number of hits 0" in r.stdout and open(out, "rb").read() == b""
    # everything is admissible at 1: clipped at the floor
    r = subprocess.run(base + ["--pssm-pvalue", "1", "--pssm-null-floor", "5"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = world["eng"].pssm_pvalue_threshold(world["loose"], 1.0, t_lo=5.0)
    names, t, _ = _read_pssm(pf2)
    assert np.array_equal(t, want["t"])
    for n, f in zip(_NAMES, want["flag"]):
        assert ("profile %s: the threshold is clipped" % n in r.stderr) == (f == 1)
    assert (want["flag"] == 1).any()


def test_pvalue_column(world):
    tmp = world["tmp"]
    out, plain = str(tmp / "col.txt"), str(tmp / "col_plain.txt")
    base = [_bin(), "-d", world["fa"], "-l", str(K), "--pssm", world["pf"]]
    r = subprocess.run(base + ["-o", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for floor in (None, FLOOR):
        r = subprocess.run(base + ["-o", out, "--pssm-pvalue-column", "1"] + (["--pssm-null-floor", floor] if floor else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        hits = world["eng"].pssm_scan(world["loose"], world["t"])
        t_lo = world["t"] if floor is None else np.minimum(world["t"], float(floor))
        pv = world["eng"].pssm_pvalue(world["loose"], hits["m"], hits["score"], t_lo=t_lo, want_lower=False)
        lines, plain_lines = open(out).read().splitlines(), open(plain).read().splitlines()
        assert len(lines) == len(plain_lines) == len(hits["m"]) > 0
        for line, pl, p_hi in zip(lines, plain_lines, pv["p_hi"]):
            assert line == pl + " %.17g" % p_hi
        assert np.all(pv["p_hi"] > 0) and np.all(pv["p_hi"] <= 1)
    # with --pssm-pvalue beside it: the thresholds of P, and every line's p_hi at most P
    pf2 = str(tmp / "col.pssm")
    r = subprocess.run(base + ["-o", out, "--pssm-pvalue-column", "1", "--pssm-pvalue", P, "--pssm-null-floor", FLOOR,
                               "--pssm-out", pf2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    col = [float(line.split(" ")[-1]) for line in open(out).read().splitlines()]
    assert len(col) > 0 and max(col) <= float(P)


def test_refusals(world):
    out, pf2 = str(world["tmp"] / "none_p.txt"), str(world["tmp"] / "none_p.pssm")
    base = [_bin(), "-d", world["fa"], "-l", str(K), "-o", out]

    def refused(args, *words):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and all(w in r.stderr for w in ("ERROR:",) + words), (args, r.stderr)

    search = ["-c", world["fa"], "-W", "100", "-T", "30"]
    refused(search + ["--pssm-pvalue", "0.01", "--pssm-out", pf2], "--pssm-pvalue", "--pssm")    # without --pssm
    refused(search + ["--pssm-pvalue-column", "1"], "--pssm-pvalue-column", "--pssm")
    refused(search + ["--pssm-null-floor", "0"], "--pssm-null-floor", "--pssm")
    refused(["--pssm", world["pf"], "--pssm-pvalue", "0.01"], "--pssm-pvalue", "--pssm-out")      # without --pssm-out
    refused(["--pssm", world["pf"], "--pssm-out", pf2], "--pssm-out", "--pssm-refine")            # stays refused
    refused(["--pssm", world["pf"], "--pssm-pvalue", "0.01", "--pssm-out", pf2, "--pssm-rank", "5"], "--pssm-pvalue",
            "--pssm-rank")
    refused(["--pssm", world["pf"], "--pssm-pvalue", "0.01", "--pssm-out", pf2, "--pssm-refine", "2"], "--pssm-pvalue",
            "--pssm-refine")
    for bad in ("0", "-0.5", "1.5", "x", "nan", "inf", "", "0.1x"):
        refused(["--pssm", world["pf"], "--pssm-pvalue", bad, "--pssm-out", pf2], "--pssm-pvalue")
    for bad in ("x", "nan", "inf", ""):
        refused(["--pssm", world["pf"], "--pssm-pvalue", "0.01", "--pssm-out", pf2, "--pssm-null-floor", bad],
                "--pssm-null-floor")
    refused(["--pssm", world["pf"], "--pssm-null-floor", "0"], "--pssm-null-floor")              # nothing to floor
    refused(["--pssm", world["pf"], "--pssm-pvalue-column", "1", "--pssm-top", "3"], "--pssm-pvalue-column", "--pssm-top")
    refused(["--pssm", world["pf"], "--pssm-pvalue-column", "1", "--pssm-per-sequence", "1"], "--pssm-pvalue-column",
            "--pssm-per-sequence")
    # what --pssm refuses stays refused with the new flag beside it
    for flag, value in (("--per-sequence", "1"), ("--topk", "3"), ("--gpus", "2")):
        refused(["--pssm", world["pf"], "--pssm-pvalue", "0.01", "--pssm-out", pf2, flag, value], "--pssm", flag)
    refused(["--pssm", world["pf"], "--pssm-pvalue", "0.01", "--pssm-out", pf2, "--pssm-per-sequence", "1", "--pssm-top",
             "3"], "--pssm-per-sequence", "--pssm-top")
