"""`hs_motif_both_points --pssm FILE --pssm-top N` on the GPU over a small FASTA database: the written lines are parsed
back and compared with the numpy contract (tests/pssm_topk_ref.py) over the database's windows -- profile, window, score
bit for bit, in order, the file's thresholds as floors -- and with the host rule (capi.pssm_topk_hits); and the two
refusals the flag adds."""
import subprocess

import numpy as np
import pytest

from hsearch_amd import capi
from tests import pssm_ref
from tests import pssm_topk_ref as ref
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"
_K = 9


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pssm_topk_cli")
    rng = np.random.default_rng(43)
    lens = [30, 4, 9, 120, 8, 61]
    seqs = ["".join(_LETTERS[c] for c in rng.integers(0, 20, n)) for n in lens]
    seqs[3] = seqs[3][:50] + "X" + seqs[3][51:]     # a letter outside the alphabet: no window crosses it
    fa = str(tmp / "db.fa")
    with open(fa, "w") as f:
        for s, seq in enumerate(seqs):
            f.write(">prot%d some description\n%s\n" % (s, seq))
    wins = [(s, off) for s, seq in enumerate(seqs) for off in range(len(seq) - _K + 1) if "X" not in seq[off:off + _K]]
    codes = np.array([[_LETTERS.index(c) for c in seqs[s][off:off + _K]] for s, off in wins], dtype=np.uint8)
    S = rng.normal(0, 1.5, size=(5, _K, 20))
    S[1] = rng.integers(-2, 3, size=(_K, 20)) / 2.0   # few distinct scores: the window index decides
    S[2, :, 3] = -1e30
    sc = pssm_ref.scores(S, codes)
    t = np.full(5, -1e300)                          # no floor to speak of
    t[3] = np.sort(sc[3])[-2]                       # a floor that leaves two windows
    t[4] = 1e9                                      # ... and one that leaves none
    names = ["motif%d" % i for i in range(5)]
    pf = str(tmp / "profiles.pssm")
    with open(pf, "w") as f:
        for nm, prof, thr in zip(names, S, t):
            f.write(">%s %r\n" % (nm, float(thr)))
            for row in prof:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
    return dict(tmp=tmp, fa=fa, pf=pf, seqs=seqs, wins=wins, codes=codes, S=S, t=t, sc=sc, names=names)


@pytest.mark.parametrize("top", [3, 64])
def test_top_lines(world, top):
    out = str(world["tmp"] / ("top%d.txt" % top))
    r = subprocess.run([_bin(), "-d", world["fa"], "-l", str(_K), "--pssm", world["pf"], "--pssm-top", str(top), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ref.rows_from_scores(world["sc"], top, world["t"])
    assert want["count"].tolist() == [top, top, top, 2, 0]
    # the host rule over every (profile, window) pair at or above the floor is the same reference
    m, i = np.nonzero(world["sc"] >= world["t"][:, None])
    ref.same_rows(capi.pssm_topk_hits(m, i, world["sc"][m, i], 5, top), want)
    lines = open(out).read().splitlines()
    assert len(lines) == int(want["count"].sum()) and "number of hits %d" % len(lines) in r.stdout
    at = 0
    for p in range(5):
        for rank in range(int(want["count"][p])):
            name, window, score = lines[at].split(" ")
            at += 1
            i = int(want["id"][p, rank])
            s, off = world["wins"][i]
            assert name == world["names"][p]
            assert window == "prot%d#%d$%d@%s*%d" % (s, s, off, world["seqs"][s][off:off + _K], i)
            assert np.float64(score).view(np.uint64) == want["score"][p, rank].view(np.uint64), lines[at - 1]
    if top == 64:   # 64 entries over at most 37 distinct scores: ties, decided by the window index
        tied = want["score"][1]
        assert (tied[1:] == tied[:-1]).any()


def test_refusals(world):
    out = str(world["tmp"] / "none.txt")
    base = [_bin(), "-d", world["fa"], "-l", str(_K), "-o", out]
    for n in ("0", "65", "-1", "x", "3x"):
        r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-top", n], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "ERROR: --pssm-top" in r.stderr and "1..64" in r.stderr, (n, r.stderr)
    r = subprocess.run(base + ["--pssm-top", "3", "-c", world["fa"], "-W", "100", "-T", "30"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "ERROR: --pssm-top" in r.stderr and "--pssm" in r.stderr
    # what --pssm refuses stays refused with the new flag beside it
    r = subprocess.run(base + ["--pssm", world["pf"], "--pssm-top", "3", "--topk", "3"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "ERROR: --pssm" in r.stderr and "--topk" in r.stderr
