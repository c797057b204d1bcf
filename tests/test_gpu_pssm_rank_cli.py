"""`hs_motif_both_points --pssm FILE --pssm-rank N --pssm-out FILE2` on the GPU over the planted-family FASTA database
of tests/test_gpu_pssm_refine_cli.py: FILE2 is FILE with every threshold replaced by Engine.pssm_rank's, bit for bit and
the matrices untouched; the -o file is byte for byte what a run with --pssm FILE2 writes (with --pssm-top and
--pssm-per-sequence too); with --pssm-refine beside it FILE2 holds Engine.pssm_refine_rank's matrices and thresholds;
and the refused flag combinations."""
import subprocess

import numpy as np
import pytest

from tests import pssm_rank_ref as ref
from tests import pssm_ref
from tests.test_gpu_pssm_counts import K
from tests.test_gpu_pssm_refine_cli import _NAMES, _read_pssm, world  # noqa: F401  (world: the module's fixture)
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

RANK = 30


@pytest.mark.parametrize("mode", ["hits", "per-sequence", "top"])
def test_ranked_file_and_output(world, mode):
    tmp = world["tmp"]
    out, out2, pf2 = str(tmp / (mode + "_r.txt")), str(tmp / (mode + "_r2.txt")), str(tmp / (mode + "_r.pssm"))
    extra = {"hits": [], "per-sequence": ["--pssm-per-sequence", "1"], "top": ["--pssm-top", "3"]}[mode]
    base = [_bin(), "-d", world["fa"], "-l", str(K)]
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-rank", str(RANK), "--pssm-out", pf2, "-o", out] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = world["eng"].pssm_rank(world["loose"], RANK)
    ref.same(want, ref.from_scores(pssm_ref.scores(world["loose"], world["codes"]), RANK), "the engine against the rule")
    names, t, S = _read_pssm(pf2)
    assert names == _NAMES and np.array_equal(t.view(np.uint64), want["t"].view(np.uint64))
    assert np.array_equal(S.view(np.uint64), world["loose"].view(np.uint64))       # the matrices as FILE gives them
    assert not np.array_equal(t, world["t"])
    r = subprocess.run(base + ["--pssm", pf2, "-o", out2] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(out, "rb").read()
    assert got == open(out2, "rb").read()
    if mode == "hits":       # exactly the rank best windows and their ties, per profile
        assert len(got.splitlines()) == int(want["cnt_ge"].sum()) >= 3 * RANK
        assert "number of hits %d" % int(want["cnt_ge"].sum()) in r.stdout


@pytest.mark.parametrize("one", [False, True])
def test_with_refine(world, one):
    tmp = world["tmp"]
    tag = "rr%d" % one
    out, out2, pf2 = str(tmp / (tag + ".txt")), str(tmp / (tag + "2.txt")), str(tmp / (tag + ".pssm"))
    base = [_bin(), "-d", world["fa"], "-l", str(K)]
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-rank", str(RANK), "--pssm-refine", "8", "--pssm-out", pf2,
                               "-o", out] + (["--pssm-one-per-protein", "1", "--pssm-pseudo", "0.5"] if one else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = world["eng"].pssm_refine_rank(world["loose"], RANK, 8, world["id_start"] if one else None,
                                         pseudo=0.5 if one else 1.0)
    assert want["converged"] and "refined in %d scans (converged)" % want["iters"] in r.stdout
    names, t, S = _read_pssm(pf2)
    assert names == _NAMES and np.array_equal(t.view(np.uint64), want["t"].view(np.uint64))
    assert np.array_equal(S.view(np.uint64), want["S"].view(np.uint64)) and not np.array_equal(S[0], world["loose"][0])
    r = subprocess.run(base + ["--pssm", pf2, "-o", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(out, "rb").read()
    assert got == open(out2, "rb").read() and len(got.splitlines()) >= 3 * RANK


def test_refusals(world):
    out, pf2 = str(world["tmp"] / "none_r.txt"), str(world["tmp"] / "none_r.pssm")
    base = [_bin(), "-d", world["fa"], "-l", str(K), "-o", out]
    n = len(world["codes"])

    def refused(args, *words):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and all(w in r.stderr for w in ("ERROR:",) + words), (args, r.stderr)

    search = ["-c", world["fa"], "-W", "100", "-T", "30"]
    refused(search + ["--pssm-rank", "5", "--pssm-out", pf2], "--pssm-rank", "--pssm")          # without --pssm
    refused(["--pssm", world["pf"], "--pssm-rank", "5"], "--pssm-rank", "--pssm-out")           # without --pssm-out
    refused(["--pssm", world["pf"], "--pssm-out", pf2], "--pssm-out", "--pssm-refine")          # stays refused
    for bad in ("0", "-1", "x", "1.5", "3e2", ""):
        refused(["--pssm", world["pf"], "--pssm-rank", bad, "--pssm-out", pf2], "--pssm-rank")
    refused(["--pssm", world["pf"], "--pssm-rank", str(n + 1), "--pssm-out", pf2], "rank")        # above the windows
    refused(["--pssm", world["pf"], "--pssm-rank", str(n + 1), "--pssm-refine", "2", "--pssm-out", pf2], "rank")
    # what --pssm refuses stays refused with the new flag beside it
    for flag, value in (("--per-sequence", "1"), ("--topk", "3"), ("--gpus", "2")):
        refused(["--pssm", world["pf"], "--pssm-rank", "5", "--pssm-out", pf2, flag, value], "--pssm", flag)
    refused(["--pssm", world["pf"], "--pssm-rank", "5", "--pssm-out", pf2, "--pssm-per-sequence", "1", "--pssm-top", "3"],
            "--pssm-per-sequence", "--pssm-top")
    refused(["--pssm", world["pf"], "--pssm-rank", "5", "--pssm-out", pf2, "--pssm-one-per-protein", "1"],
            "--pssm-one-per-protein")
    # the largest rank is accepted: every window is a hit
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-rank", str(n), "--pssm-out", pf2], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "number of hits %d" % (3 * n) in r.stdout, r.stdout + r.stderr
