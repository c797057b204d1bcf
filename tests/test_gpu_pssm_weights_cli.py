"""`hs_motif_both_points --pssm FILE --pssm-refine N --pssm-weights sites|columns --pssm-out FILE2` on the GPU over the
planted-family FASTA database of tests/test_gpu_pssm_refine_cli.py: FILE2 parses to Engine.pssm_refine_weighted's
profiles (and, with --pssm-rank, thresholds) bit for bit, the -o file is byte for byte what a run with --pssm FILE2
writes, with or without --pssm-rank and --pssm-one-per-protein, and the refused flag combinations."""
import subprocess

import numpy as np
import pytest

from tests.test_gpu_pssm_counts import K
from tests.test_gpu_pssm_refine_cli import _NAMES, _read_pssm, world  # noqa: F401  (world: the module's fixture)
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("neff", ["sites", "columns"])
@pytest.mark.parametrize("by_rank", [False, True])
@pytest.mark.parametrize("one", [False, True])
def test_weighted_file_and_output(world, neff, by_rank, one):
    tmp = world["tmp"]
    tag = "w_%s_%d_%d" % (neff, by_rank, one)
    out, out2, pf2 = str(tmp / (tag + ".txt")), str(tmp / (tag + "2.txt")), str(tmp / (tag + ".pssm"))
    base = [_bin(), "-d", world["fa"], "-l", str(K)]
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-refine", "8", "--pssm-weights", neff, "--pssm-out", pf2,
                               "-o", out] + (["--pssm-rank", "30"] if by_rank else [])
                       + (["--pssm-one-per-protein", "1", "--pssm-pseudo", "0.5"] if one else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    how = dict(rank=30) if by_rank else dict(t=world["t"])
    want = world["eng"].pssm_refine_weighted(world["loose"], 8, id_start=world["id_start"] if one else None,
                                             pseudo=0.5 if one else 1.0, neff=neff, **how)
    assert "refined in %d scans%s" % (want["iters"], " (converged)" if want["converged"] else "") in r.stdout
    names, t, S = _read_pssm(pf2)
    assert names == _NAMES
    assert np.array_equal(t.view(np.uint64), (want["t"] if by_rank else world["t"]).view(np.uint64))
    assert np.array_equal(S.view(np.uint64), want["S"].view(np.uint64))
    assert not np.array_equal(S[0], world["loose"][0])
    # the weights show: the unweighted loop writes other matrices
    plain = (world["eng"].pssm_refine_rank(world["loose"], 30, 8, world["id_start"] if one else None,
                                           pseudo=0.5 if one else 1.0) if by_rank else
             world["eng"].pssm_refine(world["loose"], world["t"], 8, world["id_start"] if one else None,
                                      pseudo=0.5 if one else 1.0))
    assert not np.array_equal(plain["S"][0], S[0])
    r = subprocess.run(base + ["--pssm", pf2, "-o", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(out, "rb").read()
    assert got == open(out2, "rb").read() and len(got.splitlines()) >= 30


def test_refusals(world):
    out, pf2 = str(world["tmp"] / "wnone.txt"), str(world["tmp"] / "wnone.pssm")
    base = [_bin(), "-d", world["fa"], "-l", str(K), "-o", out]

    def refused(args, *words):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and all(w in r.stderr for w in ("ERROR:",) + words), (args, r.stderr)

    search = ["-c", world["fa"], "-W", "100", "-T", "30"]
    refused(search + ["--pssm-weights", "sites"], "--pssm-weights", "--pssm")                        # without --pssm
    refused(["--pssm", world["pf"], "--pssm-weights", "sites"], "--pssm-weights", "--pssm-refine")  # without --pssm-refine
    refused(["--pssm", world["pf"], "--pssm-rank", "30", "--pssm-out", pf2, "--pssm-weights", "columns"],
            "--pssm-weights", "--pssm-refine")
    for v in ("site", "Sites", "1", "none", ""):
        refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-out", pf2, "--pssm-weights", v], "--pssm-weights",
                "'sites' or 'columns'")
    refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-weights", "sites"], "--pssm-refine", "--pssm-out")
    # what --pssm refuses stays refused with the new flag beside it
    for flag, value in (("--per-sequence", "1"), ("--topk", "3"), ("--gpus", "2")):
        refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-out", pf2, "--pssm-weights", "sites", flag, value],
                "--pssm", flag)
    refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-out", pf2, "--pssm-weights", "sites",
             "--pssm-pvalue", "0.01"], "--pssm-pvalue")
