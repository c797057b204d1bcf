"""`hs_motif_both_points --pssm FILE --pssm-per-sequence 1` on the GPU over a small FASTA database: the written lines
are parsed back and compared with the numpy rule (tests/pssm_seq_ref.py) over the database's windows -- profile,
protein, count, best window and its score bit for bit, span, profiles in file order and proteins in database order --
and the refusals the flag adds."""
import subprocess

import numpy as np
import pytest

from tests import pssm_ref
from tests import pssm_seq_ref as ref
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"
_K = 9


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pssm_seq_cli")
    rng = np.random.default_rng(47)
    lens = [30, 4, 9, 120, 8, 61, 200]                # (shorter than k, exactly k: proteins without and with one window)
    seqs = ["".join(_LETTERS[c] for c in rng.integers(0, 20, n)) for n in lens]
    seqs[3] = seqs[3][:50] + "X" + seqs[3][51:]     # a letter outside the alphabet: no window crosses it
    fa = str(tmp / "db.fa")
    with open(fa, "w") as f:
        for s, seq in enumerate(seqs):
            f.write(">prot%d some description\n%s\n" % (s, seq))
    wins = [(s, off) for s, seq in enumerate(seqs) for off in range(len(seq) - _K + 1) if "X" not in seq[off:off + _K]]
    codes = np.array([[_LETTERS.index(c) for c in seqs[s][off:off + _K]] for s, off in wins], dtype=np.uint8)
    per = np.bincount([s for s, _ in wins], minlength=len(seqs))
    id_start = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    S = rng.normal(0, 1.5, size=(5, _K, 20))
    S[1] = 0.0                                        # scores 0, 1 or 2: the best of a protein is tied many times over
    S[1, 0, :10] = S[1, 4, :10] = 1.0
    sc = pssm_ref.scores(S, codes)
    t = np.sort(sc, axis=1)[:, -30].copy()
    t[0] = -1e300                                     # every window hits
    t[1] = 1.0
    t[4] = 1e9                                        # no window hits
    # out of name order: the lines follow the file
    names = ["zeta", "motif1", "alpha", "motif3", "motif4"]
    pf = str(tmp / "profiles.pssm")
    with open(pf, "w") as f:
        for nm, prof, thr in zip(names, S, t):
            f.write(">%s %r\n" % (nm, float(thr)))
            for row in prof:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
    return dict(tmp=tmp, fa=fa, pf=pf, seqs=seqs, wins=wins, codes=codes, S=S, t=t, sc=sc, names=names,
                id_start=id_start, per=per)


def test_per_sequence_lines(world):
    out = str(world["tmp"] / "rows.txt")
    r = subprocess.run([_bin(), "-d", world["fa"], "-l", str(_K), "--pssm", world["pf"], "--pssm-per-sequence", "1",
                        "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ref.rows(pssm_ref.scan(world["S"], world["t"], world["codes"]), 5, world["id_start"])
    with_windows = np.flatnonzero(world["per"] > 0)
    assert want["seq"][want["m"] == 0].tolist() == with_windows.tolist() and want["seq_cnt"][4] == 0
    lines = open(out).read().splitlines()
    assert len(lines) == len(want["m"]) >= 10
    assert "number of hits %d" % want["n_hits"] in r.stdout and "number of rows %d" % len(lines) in r.stdout
    tied = 0
    for i, line in enumerate(lines):
        name, protein, count, best_off, score, first, last = line.split(" ")
        s = int(want["seq"][i])
        w0 = int(world["id_start"][s])
        assert name == world["names"][want["m"][i]] and protein == "prot%d#%d" % (s, s), line
        assert int(count) == want["count"][i]
        assert world["wins"][int(want["best_id"][i])] == (s, int(best_off)), line
        assert np.float64(score).view(np.uint64) == want["best_score"][i].view(np.uint64), line
        assert world["wins"][w0 + int(want["lo"][i])] == (s, int(first)), line
        assert world["wins"][w0 + int(want["hi"][i])] == (s, int(last)), line
        row = world["sc"][want["m"][i], w0:int(world["id_start"][s + 1])]
        tied += int((row == want["best_score"][i]).sum() > 1)
    assert tied >= 2
    # protein 3 holds the cut: its window offsets jump over the X at residue 50
    all3 = [l.split(" ") for l in lines if l.startswith("zeta prot3#3 ")]
    assert len(all3) == 1 and all3[0][2] == str(120 - _K + 1 - _K) and all3[0][5:] == ["0", str(120 - _K)]


def test_refusals(world):
    out = str(world["tmp"] / "none.txt")
    base = [_bin(), "-d", world["fa"], "-l", str(_K), "-o", out]
    r = subprocess.run(base + ["--pssm-per-sequence", "1", "-c", world["fa"], "-W", "100", "-T", "30"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "ERROR: --pssm-per-sequence" in r.stderr and "--pssm" in r.stderr
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-per-sequence", "1", "--pssm-top", "3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "ERROR: --pssm-per-sequence" in r.stderr and "--pssm-top" in r.stderr
    # what --pssm refuses stays refused with the new flag beside it: --per-sequence among them
    for flag, value in (("--per-sequence", "1"), ("--topk", "3"), ("--gpus", "2")):
        r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-per-sequence", "1", flag, value], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode != 0 and "ERROR: --pssm" in r.stderr and flag in r.stderr, (flag, r.stderr)
