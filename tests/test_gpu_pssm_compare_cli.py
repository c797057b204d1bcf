"""`hs_motif_both_points -l k --pssm FILE --pssm-compare FILE2|self --pssm-compare-threshold T -o OUT` on the GPU: OUT
byte for byte from the host rule (capi.pssm_compare_columns + capi.pssm_compare_host) under every column transform and
an overlap; `self` against two copies of one file; every refused combination; and a plain --pssm scan beside it, its
lines those of Engine.pssm_scan."""
import subprocess

import numpy as np
import pytest

from hsearch_amd import capi
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

K, A = 25, 20


def _write_pssm(path, names, S, t=0.0):
    with open(str(path), "w") as f:
        for nm, prof in zip(names, S):
            f.write(">%s %.17g\n" % (nm, t))
            for row in prof:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    return str(path)


def _families(seed, n_fam, members, extra):
    """profiles cut from shared masters at shifts of 3 columns, with noise, and unrelated ones"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_fam):
        master = rng.normal(0, 1, size=(K + 3 * members, A))
        for j in range(members):
            out.append(master[3 * j:3 * j + K] + rng.normal(0, 0.3, size=(K, A)))
    for _ in range(extra):
        out.append(rng.normal(0, 1, size=(K, A)))
    return np.array(out)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pssm_compare_cli")
    X, Y = _families(1, 3, 4, 9), _families(1, 3, 4, 0)[::-1].copy()      # Y: X's families, in another order
    nx, ny = ["x%d" % i for i in range(len(X))], ["y%d" % i for i in range(len(Y))]
    return dict(tmp=tmp, X=X, Y=Y, nx=nx, ny=ny, fx=_write_pssm(tmp / "x.pssm", nx, X), fy=_write_pssm(tmp / "y.pssm", ny, Y))


def _expected(X, nx, Y, ny, T, v, columns):
    if columns != "raw":
        X = capi.pssm_compare_columns(X, columns)
        Y = capi.pssm_compare_columns(Y, columns) if Y is not None else None
    h = capi.pssm_compare_host(X, T, Y, v)
    names_y = ny if Y is not None else nx
    return "".join("%s %s %d %.17g\n" % (nx[x], names_y[y], d, s) for x, y, d, s in zip(h["x"], h["y"], h["d"], h["score"]))


@pytest.mark.parametrize("columns,T,v", [(None, 0.5 * K, 1), ("pearson", 0.4 * K, 13), ("cosine", 0.5 * K, 13),
                                         ("raw", 200.0, K)])
def test_output_equals_host_rule(files, columns, T, v):
    out = str(files["tmp"] / ("out_%s.txt" % columns))
    cmd = [_bin(), "-l", str(K), "--pssm", files["fx"], "--pssm-compare", files["fy"], "--pssm-compare-threshold",
           "%.17g" % T, "-o", out]
    if columns:
        cmd += ["--pssm-compare-columns", columns]
    if v != 1:
        cmd += ["--pssm-compare-overlap", str(v)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = _expected(files["X"], files["nx"], files["Y"], files["ny"], T, v, columns or "pearson")
    got = open(out).read()
    assert got == want and len(want.splitlines()) >= 3
    assert "number of hits %d" % len(want.splitlines()) in r.stdout


def test_self_equals_two_copies(files):
    tmp = files["tmp"]
    out_self, out_two = str(tmp / "self.txt"), str(tmp / "two.txt")
    base = [_bin(), "-l", str(K), "--pssm", files["fx"], "--pssm-compare-threshold", "10", "--pssm-compare-overlap", "13"]
    r = subprocess.run(base + ["--pssm-compare", "self", "-o", out_self], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    copy = _write_pssm(tmp / "x_copy.pssm", files["nx"], files["X"])
    r = subprocess.run(base + ["--pssm-compare", copy, "-o", out_two], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    order = {n: i for i, n in enumerate(files["nx"])}
    upper = [l for l in open(out_two).read().splitlines(True) if order[l.split()[0]] < order[l.split()[1]]]
    got = open(out_self).read()
    assert got == "".join(upper) == _expected(files["X"], files["nx"], None, None, 10.0, 13, "pearson")
    assert len(upper) >= 9                                        # the pairs of shifts of three families


def test_refusals(files):
    tmp = files["tmp"]
    out = str(tmp / "refused.txt")
    ok = ["-l", str(K), "--pssm", files["fx"], "--pssm-compare", files["fy"], "--pssm-compare-threshold", "12", "-o", out]

    def refused(args, *words):
        r = subprocess.run([_bin()] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "ERROR" in r.stderr, (args, r.stdout, r.stderr)
        for w in words:
            assert w in r.stderr, (w, r.stderr)
        assert not (tmp / "refused.txt").exists()

    def without(args, flag):
        i = args.index(flag)
        return args[:i] + args[i + 2:]

    refused(without(ok, "--pssm"), "--pssm-compare", "--pssm")
    refused(without(ok, "--pssm-compare-threshold"), "--pssm-compare-threshold")
    refused(without(without(ok, "--pssm-compare"), "--pssm-compare-threshold") + ["-d", files["fx"], "--pssm-compare-overlap", "3"],
            "--pssm-compare-overlap", "--pssm-compare")
    for flag, value in (("--pssm-rank", "5"), ("--pssm-refine", "2"), ("--pssm-pvalue", "0.01"), ("--pssm-top", "3"),
                        ("--pssm-per-sequence", "1")):
        refused(ok + [flag, value] + (["--pssm-out", str(tmp / "o.pssm")] if flag in ("--pssm-rank", "--pssm-refine", "--pssm-pvalue") else []),
                "--pssm-compare", flag)
    for bad in ("0", str(K + 1), "-1", "x", "1.5"):
        refused(ok + ["--pssm-compare-overlap", bad], "--pssm-compare-overlap")
    for bad in ("spearman", "", "Pearson"):
        refused(ok + ["--pssm-compare-columns", bad], "--pssm-compare-columns")
    for bad in ("nan", "inf", "x", ""):
        refused(without(ok, "--pssm-compare-threshold") + ["--pssm-compare-threshold", bad], "--pssm-compare-threshold")
    # files of another k or another alphabet
    short = _write_pssm(tmp / "short.pssm", ["s0"], files["X"][:1, :K - 1])
    narrow = _write_pssm(tmp / "narrow.pssm", ["n0"], files["X"][:1, :, :A - 1])
    refused(without(ok, "--pssm-compare") + ["--pssm-compare", short], "short.pssm")
    refused(without(ok, "--pssm-compare") + ["--pssm-compare", narrow], "narrow.pssm")
    refused(without(ok, "--pssm") + ["--pssm", narrow], "narrow.pssm")
    refused(without(ok, "--pssm-compare") + ["--pssm-compare", str(tmp / "missing.pssm")], "missing.pssm")
    # what --pssm refuses stays refused
    refused(ok + ["-c", files["fx"]], "--pssm", "-c")
    refused(ok + ["--topk", "3"], "--pssm", "--topk")
    refused(ok + ["--gpus", "2"], "--pssm", "--gpus")
    # a value the library refuses
    big = files["X"][:1].copy()
    big[0, 0, 0] = 3e30
    refused(without(ok, "--pssm-compare") + ["--pssm-compare", _write_pssm(tmp / "big.pssm", ["b0"], big),
                                              "--pssm-compare-columns", "raw"], "2^100")


def test_a_plain_pssm_scan_beside_it(files):
    """an existing invocation: --pssm over a FASTA database writes Engine.pssm_scan's hits, as it did"""
    from hsearch_amd import Engine, synth
    tmp = files["tmp"]
    rng = np.random.default_rng(4)
    letters = capi.alphabet()
    codes = [rng.integers(0, A, size=n) for n in (60, 25, 140, 31)]
    seqs = ["".join(letters[c] for c in row) for row in codes]
    fa = tmp / "db.fa"
    fa.write_text("".join(">p%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    S = rng.integers(-8, 9, size=(3, K, A)) / 4.0
    names = ["m0", "m1", "m2"]
    pf, out = _write_pssm(tmp / "scan.pssm", names, S, t=4.0), str(tmp / "scan.txt")
    r = subprocess.run([_bin(), "-d", str(fa), "-l", str(K), "--pssm", pf, "-o", out], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    windows = np.array([c[p:p + K] for c in codes for p in range(len(c) - K + 1)], dtype=np.uint8)
    a, b = synth.make_planes(K, 2, 1, 200.0, seed=3)
    eng = Engine(K, 2, 1, 200.0, a, b)
    try:
        eng.index_build(windows)
        hits = eng.pssm_scan(S, np.full(3, 4.0))
    finally:
        eng.close()
    lines = open(out).read().splitlines()
    assert len(lines) == len(hits["m"]) > 0
    for line, m, wid, sc in zip(lines, hits["m"], hits["id"], hits["score"]):
        tok = line.split()
        assert tok[0] == names[m] and tok[1].endswith("*%d" % wid) and tok[2] == "%.17g" % sc, line
