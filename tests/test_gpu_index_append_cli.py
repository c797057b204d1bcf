"""`hs_motif_both_points --db-append FASTA` on the GPU: the database is the -d file's windows followed by each
appended file's (the index grown by hs_index_append_windows), sequence numbers and names continuing -- so the output
must equal, line for line, a run over the concatenated FASTA file: the plain hit list, --per-sequence 1, --topk N
and --best-per-position 1.  And the two refusals: a points database, several GPUs."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_components_cli import _LETTERS
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

_K = 25


def _proteins(rng, motif, lengths, prefix):
    """FASTA text: proteins that share a mutated stretch (windows of different files in one bucket)"""
    out = []
    for i, n in enumerate(lengths):
        s = rng.integers(0, 20, size=n)
        if n >= 90:
            s[10:70] = motif
            s[rng.integers(10, 70, size=3)] = rng.integers(0, 20, size=3)
        text = "".join(_LETTERS[c] for c in s)
        if n == 131:
            text = text[:80] + "X" + text[81:]      # a letter outside the alphabet: no window across it
        out.append(">%s%d from file %s\n%s\n" % (prefix, i, prefix, text))
    return "".join(out)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("append_cli")
    rng = np.random.default_rng(17)
    motif = rng.integers(0, 20, size=60)
    parts = [_proteins(rng, motif, [300, 120, 25, 200], "a"), _proteins(rng, motif, [150, 24, 131, 95], "b"),
             _proteins(rng, motif, [25, 260], "c")]
    files = []
    for name, text in zip(("a.fa", "b.fa", "c.fa"), parts):
        files.append(str(tmp / name))
        open(files[-1], "w").write(text)
    whole = str(tmp / "all.fa")
    open(whole, "w").write("".join(parts))
    cfa = str(tmp / "centres.fa")
    with open(cfa, "w") as f:    # centres: windows of the motif, mutated
        for i in range(30):
            c = motif[i:i + _K].copy()
            c[rng.integers(0, _K, size=2)] = rng.integers(0, 20, size=2)
            f.write(">c%d\n%s\n" % (i, "".join(_LETTERS[x] for x in c)))
    common = ["-c", cfa, "-l", str(_K), "-K", "6", "-L", "3", "-W", "60", "-T", "40", "--seed", "23"]
    return dict(tmp=tmp, files=files, whole=whole, common=common)


def _lines(cmd, out):
    r = subprocess.run(cmd + ["-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return open(out).read().splitlines()


@pytest.mark.parametrize("mode", [[], ["--per-sequence", "1"], ["--topk", "3"], ["--best-per-position", "1"]],
                         ids=["hits", "per-sequence", "topk", "best-per-position"])
def test_appended_files_equal_the_concatenated_file(world, mode):
    w = world
    want = _lines([_bin(), "-d", w["whole"]] + w["common"] + mode, str(w["tmp"] / "want.txt"))
    got = _lines([_bin(), "-d", w["files"][0], "--db-append", w["files"][1], "--db-append", w["files"][2]] + w["common"]
                 + mode, str(w["tmp"] / "got.txt"))
    assert len(want) > 20
    if not mode:    # hits in windows of every file, numbered on: file c's second protein is number 9
        assert any(" a0#0$" in ln for ln in want) and any(" b0#4$" in ln for ln in want)
        assert any(" c1#9$" in ln for ln in want)
    assert got == want


def test_refusals(world):
    w = world
    out = str(w["tmp"] / "never.txt")
    pts = str(w["tmp"] / "points.txt")
    with open(pts, "w") as f:
        for i in range(3):
            f.write(">p%d\n%s\n" % (i, " ".join("%d" % ((i + j) % 5) for j in range(8 * _K))))
    base = w["common"] + ["-o", out, "--db-append", w["files"][1]]
    for cmd, word in (([_bin(), "-d", pts] + base, "FASTA database"),
                      ([_bin(), "-d", w["files"][0]] + base + ["--gpus", "2"], "--gpus")):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ERROR" in r.stderr and "--db-append" in r.stderr and word in r.stderr, cmd
    assert not os.path.exists(out)
