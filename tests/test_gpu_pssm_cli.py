"""`hs_motif_both_points --pssm FILE` on the GPU over a small FASTA database: the written lines are parsed back and
compared with the numpy contract (tests/pssm_ref.py) over the database's windows -- profile, window, score bit for bit,
in order --; the file format's errors; and the refused flag combinations."""
import subprocess

import numpy as np
import pytest

from tests import pssm_ref
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"
_K = 9


def _write_pssm(path, names, S, t):
    with open(path, "w") as f:
        for nm, prof, thr in zip(names, S, t):
            f.write(">%s %r\n" % (nm, float(thr)))
            for row in prof:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pssm_cli")
    rng = np.random.default_rng(41)
    lens = [30, 4, 9, 120, 8, 61]
    seqs = ["".join(_LETTERS[c] for c in rng.integers(0, 20, n)) for n in lens]
    seqs[3] = seqs[3][:50] + "X" + seqs[3][51:]     # a letter outside the alphabet: no window crosses it
    fa = str(tmp / "db.fa")
    with open(fa, "w") as f:
        for s, seq in enumerate(seqs):
            f.write(">prot%d some description\n%s\n" % (s, seq))
    # the windows, as the scan numbers them: sequence-major, ascending offset, none across the X
    wins = [(s, off) for s, seq in enumerate(seqs) for off in range(len(seq) - _K + 1) if "X" not in seq[off:off + _K]]
    codes = np.array([[_LETTERS.index(c) for c in seqs[s][off:off + _K]] for s, off in wins], dtype=np.uint8)
    S = rng.normal(0, 1.5, size=(5, _K, 20))
    S[1] = rng.integers(-8, 9, size=(_K, 20)) / 4.0
    S[2, :, 3] = -1e30
    t = np.sort(pssm_ref.scores(S, codes), axis=1)[:, -12].copy()
    t[4] = 1e9    # no hit
    names = ["motif%d" % i for i in range(5)]
    pf = str(tmp / "profiles.pssm")
    _write_pssm(pf, names, S, t)
    return dict(tmp=tmp, fa=fa, pf=pf, seqs=seqs, wins=wins, codes=codes, S=S, t=t, names=names)


def test_scan_lines(world):
    out = str(world["tmp"] / "hits.txt")
    r = subprocess.run([_bin(), "-d", world["fa"], "-l", str(_K), "--pssm", world["pf"], "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = pssm_ref.scan(world["S"], world["t"], world["codes"])
    assert len(want["m"]) >= 48 and want["cnt"][4] == 0
    assert "number of kmers %d" % len(world["wins"]) in r.stdout and "number of hits %d" % len(want["m"]) in r.stdout
    lines = open(out).read().splitlines()
    assert len(lines) == len(want["m"])
    for line, m, i, sc in zip(lines, want["m"], want["id"], want["score"]):
        name, window, score = line.split(" ")
        s, off = world["wins"][int(i)]
        assert name == world["names"][int(m)]
        assert window == "prot%d#%d$%d@%s*%d" % (s, s, off, world["seqs"][s][off:off + _K], int(i))
        assert np.float64(score).view(np.uint64) == np.float64(sc).view(np.uint64), line


def test_file_errors(world):
    tmp = world["tmp"]
    out = str(tmp / "none.txt")

    def run(text):
        pf = str(tmp / "bad.pssm")
        with open(pf, "w") as f:
            f.write(text)
        return subprocess.run([_bin(), "-d", world["fa"], "-l", str(_K), "--pssm", pf, "-o", out], capture_output=True,
                              text=True, timeout=300)
    row = " ".join(["0.5"] * 20) + "\n"
    for text, what in ((">a 1.0\n" + row * (_K - 1), "fewer than"), (">a 1.0\n" + row * (_K + 1), "more rows"),
                       (">a\n" + row * _K, "threshold"), (">a 1.0\n" + row * (_K - 1) + " ".join(["0.5"] * 19) + "\n", "20 numbers"),
                       (">a 1.0\n" + row * (_K - 1) + " ".join(["0.5"] * 19 + ["x"]) + "\n", "not a number"),
                       (">a 1.0\n" + row * _K + ">a 2.0\n" + row * _K, "twice"), (row * _K, "threshold"),
                       (">a 1.0\n" + row * (_K - 1) + " ".join(["0.5"] * 19 + ["nan"]) + "\n", "NaN")):
        r = run(text)
        assert r.returncode != 0 and "ERROR" in r.stderr and what in r.stderr, (what, r.stderr)


def test_refusals(world):
    out = str(world["tmp"] / "none.txt")
    base = [_bin(), "-d", world["fa"], "-l", str(_K), "--pssm", world["pf"], "-o", out]
    for extra, what in ((["-c", world["fa"]], "-c"), (["--radii", world["pf"]], "--radii"), (["-M", "2"], "-M"),
                        (["--topk", "3"], "--topk"), (["--per-sequence", "1"], "--per-sequence"),
                        (["--best-per-position", "1"], "--best-per-position"),
                        (["--query-fasta", world["fa"]], "--query-fasta"), (["--gpus", "2"], "--gpus")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "ERROR: --pssm" in r.stderr and what in r.stderr, (extra, r.stderr)
    # a points database holds no residues
    pts = str(world["tmp"] / "db.points")
    with open(pts, "w") as f:
        f.write(">p0\n" + " ".join(["1.0"] * (8 * _K)) + "\n")
    r = subprocess.run([_bin(), "-d", pts, "-l", str(_K), "--pssm", world["pf"], "-o", out], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "needs a FASTA database" in r.stderr
