"""`hs_motif_both_points --pssm FILE --pssm-refine N --pssm-out FILE2` on the GPU over a planted-family FASTA database:
FILE2 parses to Engine.pssm_refine's profiles bit for bit with names and thresholds kept, the -o file is byte for byte
what a run with --pssm FILE2 writes (with --pssm-top and --pssm-per-sequence too), and the refused flag combinations."""
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, synth
from tests.test_gpu_pssm_counts import A, K, planted
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"
_NAMES = ["zeta", "family1", "nowhere"]


def _write_pssm(path, names, S, t):
    with open(path, "w") as f:
        for nm, prof, thr in zip(names, S, t):
            f.write(">%s %r\n" % (nm, float(thr)))
            for row in prof:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")


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
    return names, np.array(t), np.array(rows).reshape(len(names), K, A)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pssm_refine_cli")
    fam = planted()
    starts = fam["seq_start"].astype(np.int64)
    fa = str(tmp / "db.fa")
    with open(fa, "w") as f:
        for s in range(len(starts) - 1):
            f.write(">prot%d\n%s\n" % (s, "".join(_LETTERS[c] for c in fam["residues"][starts[s]:starts[s + 1]])))
    pf = str(tmp / "profiles.pssm")
    _write_pssm(pf, _NAMES, fam["loose"], fam["t"])
    a, b = synth.make_planes(K, 2, 1, 200.0, seed=3)
    eng = Engine(K, 2, 1, 200.0, a, b)
    eng.index_build_windows(fam["residues"], fam["seq_start"])
    yield dict(fam, tmp=tmp, fa=fa, pf=pf, eng=eng)
    eng.close()


@pytest.mark.parametrize("mode", ["hits", "per-sequence", "top"])
def test_refined_file_and_output(world, mode):
    tmp = world["tmp"]
    out, out2, pf2 = str(tmp / (mode + ".txt")), str(tmp / (mode + "2.txt")), str(tmp / (mode + ".pssm"))
    one = mode == "per-sequence"
    extra = {"hits": [], "per-sequence": ["--pssm-per-sequence", "1"], "top": ["--pssm-top", "3"]}[mode]
    base = [_bin(), "-d", world["fa"], "-l", str(K)]
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-refine", "8", "--pssm-out", pf2, "-o", out] + extra
                       + (["--pssm-one-per-protein", "1", "--pssm-pseudo", "0.5"] if one else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = world["eng"].pssm_refine(world["loose"], world["t"], 8, world["id_start"] if one else None,
                                    pseudo=0.5 if one else 1.0)
    assert want["converged"] and "refined in %d scans (converged)" % want["iters"] in r.stdout
    names, t, S = _read_pssm(pf2)
    assert names == _NAMES and np.array_equal(t.view(np.uint64), world["t"].view(np.uint64))
    assert np.array_equal(S.view(np.uint64), want["S"].view(np.uint64))
    assert np.array_equal(S[2], world["loose"][2]) and not np.array_equal(S[0], world["loose"][0])
    r = subprocess.run(base + ["--pssm", pf2, "-o", out2] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(out, "rb").read()
    assert got == open(out2, "rb").read() and len(got.splitlines()) >= (6 if mode == "top" else 40)


def test_refusals(world):
    out, pf2 = str(world["tmp"] / "none.txt"), str(world["tmp"] / "none.pssm")
    base = [_bin(), "-d", world["fa"], "-l", str(K), "-o", out]

    def refused(args, *words):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and all(w in r.stderr for w in ("ERROR:",) + words), (args, r.stderr)

    search = ["-c", world["fa"], "-W", "100", "-T", "30"]
    refused(search + ["--pssm-refine", "3", "--pssm-out", pf2], "--pssm-refine", "--pssm")       # without --pssm
    refused(search + ["--pssm-out", pf2], "--pssm-out")
    refused(["--pssm", world["pf"], "--pssm-refine", "3"], "--pssm-refine", "--pssm-out")        # without --pssm-out
    refused(["--pssm", world["pf"], "--pssm-out", pf2], "--pssm-out", "--pssm-refine")
    refused(["--pssm", world["pf"], "--pssm-one-per-protein", "1"], "--pssm-one-per-protein")
    for n in ("0", "101", "x", "-1"):
        refused(["--pssm", world["pf"], "--pssm-refine", n, "--pssm-out", pf2], "--pssm-refine", "1..100")
    for x in ("0", "-1", "inf", "nan", "y"):
        refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-out", pf2, "--pssm-pseudo", x], "--pssm-pseudo")
    # what --pssm refuses stays refused with the new flags beside it
    for flag, value in (("--per-sequence", "1"), ("--topk", "3"), ("--gpus", "2")):
        refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-out", pf2, flag, value], "--pssm", flag)
    refused(["--pssm", world["pf"], "--pssm-refine", "2", "--pssm-out", pf2, "--pssm-per-sequence", "1", "--pssm-top", "3"],
            "--pssm-per-sequence", "--pssm-top")
