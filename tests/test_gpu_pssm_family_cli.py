"""`hs_motif_both_points -d proteins.fa -l k --pssm FILE --pssm-families FAM [--pssm-family-blocks C]
[--pssm-family-threshold T] -o OUT` and `--pssm-compare self ... --pssm-families-out FAM` on the GPU: the bytes of OUT
from the host rule (capi.pssm_family_hits over tests/pssm_ref.py's scan), the bytes of FAM from
tests/pssm_family_ref.layout, the two chained over the planted motif, and every refused combination.  That
`--pssm-compare self` writes the same bytes with and without the new option is shown here between two runs of this
build; that those bytes are the host rule's, as before the option existed, rests on tests/test_gpu_pssm_compare_cli.py."""
import subprocess

import numpy as np
import pytest

from hsearch_amd import capi
from tests import pssm_family_ref as ref, pssm_ref
from tests.test_gpu_pssm_compare_cli import _write_pssm
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

K, A = 25, 20


def _run(args):
    return subprocess.run([_bin()] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The planted motif's proteins as FASTA, its three window profiles and four unrelated ones in a shuffled file
    order, and a FAM file that names two families and the loners in another order than FILE."""
    tmp = tmp_path_factory.mktemp("pssm_family_cli")
    c = ref.planted_case()
    letters = capi.alphabet()
    starts = c["seq_start"].astype(np.int64)
    prots = ["".join(letters[r] for r in c["residues"][a:b]) for a, b in zip(starts[:-1], starts[1:])]
    fa = tmp / "db.fa"
    fa.write_text("".join(">p%d some text\n%s\n" % (i, s) for i, s in enumerate(prots)))
    rng = np.random.default_rng(77)
    extra = rng.integers(-8, 9, size=(4, K, A)) / 4.0
    S = np.concatenate([extra[:2], c["S"][[2, 0, 1]], extra[2:]])            # file order: e0 e1 w6 w0 w3 e2 e3
    names = ["e0", "e1", "w6", "w0", "w3", "e2", "e3"]
    sc = pssm_ref.scores(S, c["codes"])
    t = np.array([np.sort(sc[m])[-60] if n[0] == "e" else ref.PLANTED_T for m, n in enumerate(names)])
    pf = tmp / "prof.pssm"
    with open(str(pf), "w") as f:
        for n, prof, tt in zip(names, S, t):
            f.write(">%s %.17g\n" % (n, tt))
            for row in prof:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    fam_lines = [("other", "e3", 2), ("motif", "w3", 3), ("motif", "w0", 0), ("other", "e1", 2), ("lone", "e0", 0),
                 ("motif", "w6", 6), ("other", "e2", 0)]
    fam = tmp / "fam.txt"
    fam.write_text("".join("%s %s %d\n" % l for l in fam_lines) + "\n")
    return dict(c, tmp=tmp, fa=str(fa), pf=str(pf), fam=str(fam), fam_lines=fam_lines, S7=S, t7=t, names=names)


def _expected(world, blocks=1, threshold=None):
    """OUT from the host rule: the CLI's own ordering by (family in order of first appearance, offset, file order)"""
    names = world["names"]
    fam_of = {n: f for f, n, _ in world["fam_lines"]}
    off_of = {n: o for _, n, o in world["fam_lines"]}
    fams = []
    for f, _, _ in world["fam_lines"]:
        if f not in fams:
            fams.append(f)
    order = sorted(range(len(names)), key=lambda m: (fams.index(fam_of[names[m]]), off_of[names[m]], m))
    S, t = world["S7"][order], world["t7"][order]
    m_group = np.array([fams.index(fam_of[names[m]]) for m in order], dtype=np.uint32)
    m_off = np.array([off_of[names[m]] for m in order], dtype=np.uint32)
    hits = pssm_ref.scan(S, t, world["codes"])
    rows = capi.pssm_family_hits(hits["m"], hits["id"], hits["score"], len(order), world["id_start"], m_group=m_group,
                                 m_off=m_off, min_count=blocks,
                                 t_group=None if threshold is None else np.full(len(fams), threshold))
    ids = world["id_start"].astype(np.int64)
    lines = []
    for r in range(len(rows["group"])):
        s = int(rows["seq"][r])
        lines.append("%s p%d#%d %d %d %.17g %s %d %.17g %d %d\n" % (
            fams[rows["group"][r]], s, s, rows["diag"][r], rows["count"][r], rows["sum"][r],
            names[order[rows["best_m"][r]]], int(rows["best_id"][r]) - ids[s], rows["best_score"][r], rows["lo"][r],
            rows["hi"][r]))
    return "".join(lines), rows, fams


@pytest.mark.parametrize("blocks,threshold", [(None, None), (2, None), (3, None), (1, 60.0), (2, -5.5)])
def test_output_equals_host_rule(world, blocks, threshold):
    out = str(world["tmp"] / ("out_%s_%s.txt" % (blocks, threshold)))
    cmd = ["-d", world["fa"], "-l", str(K), "--pssm", world["pf"], "--pssm-families", world["fam"], "-o", out]
    if blocks is not None:
        cmd += ["--pssm-family-blocks", str(blocks)]
    if threshold is not None:
        cmd += ["--pssm-family-threshold", "%.17g" % threshold]
    r = _run(cmd)
    assert r.returncode == 0, r.stdout + r.stderr
    want, rows, fams = _expected(world, blocks or 1, threshold)
    assert open(out).read() == want
    assert "number of rows %d" % len(rows["group"]) in r.stdout and "in 3 families" in r.stdout
    if blocks is None and threshold is None:
        assert set(rows["group"].tolist()) == {0, 1, 2} and (rows["diag"] < 0).any()     # families in FAM order
    if blocks == 3:       # the motif family alone has three profiles on a diagonal: the planted proteins
        motif = rows["group"] == fams.index("motif")
        assert dict(zip(rows["seq"][motif].tolist(), rows["diag"][motif].tolist())) == world["planted"]
    assert len(want.splitlines()) >= (5 if threshold != 60.0 else 1)


def test_families_out_and_the_chain(world):
    """--pssm-compare self --pssm-families-out writes the layout of the compare hits; the compare output itself is
    byte for byte what the run without the option writes; FAM fed back with --pssm-family-blocks 3 reports the planted
    proteins."""
    tmp = world["tmp"]
    plain, with_fam, fam = str(tmp / "cmp.txt"), str(tmp / "cmp_fam.txt"), str(tmp / "fam_out.txt")
    base = ["-l", str(K), "--pssm", world["pf"], "--pssm-compare", "self", "--pssm-compare-threshold", "10",
            "--pssm-compare-overlap", "13"]
    r0 = _run(base + ["-o", plain])
    r1 = _run(base + ["-o", with_fam, "--pssm-families-out", fam])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert open(plain).read() == open(with_fam).read() and len(open(plain).read().splitlines()) == 3
    assert "number of families" not in r0.stdout and "number of families 5" in r1.stdout and "NOTE" not in r1.stderr
    names = world["names"]
    h = capi.pssm_compare_host(capi.pssm_compare_columns(world["S7"], "pearson"), 10.0, None, 13)
    lay = ref.layout(h["x"], h["y"], h["d"], len(names))
    first = {}
    for m in lay["order"]:
        first.setdefault(int(lay["group"][m]), names[m])
    want = "".join("%s %s %d\n" % (first[int(lay["group"][m])], names[m], lay["off"][m]) for m in lay["order"])
    assert open(fam).read() == want
    assert "w0 w0 0\nw0 w3 3\nw0 w6 6\n" in want and want.startswith("e0 e0 0\n")
    out = str(tmp / "chain.txt")
    r = _run(["-d", world["fa"], "-l", str(K), "--pssm", world["pf"], "--pssm-families", fam, "--pssm-family-blocks", "3",
              "-o", out])
    assert r.returncode == 0, r.stdout + r.stderr
    got = [l.split() for l in open(out).read().splitlines()]
    assert {int(l[1].split("#")[1]): int(l[2]) for l in got} == world["planted"] and all(l[0] == "w0" for l in got)
    assert len(got) == 9 and all(l[3] == "3" for l in got)
    # A contradiction is counted on stderr.  Profile r: columns 0..11 are the motif's first twelve (r lies at w0's
    # place), columns 12..23 the motif's from 19 on (r lies one column right of w6, at 7): both hits come, the second
    # one to be taken disagrees with the first.
    motif = world["motif"]
    res = np.concatenate([motif[:12], motif[19:31], [(motif[24] + 1) % A]])
    R = np.full((1, K, A), -1.0)
    R[0, np.arange(K), res] = 2.0
    S8 = np.concatenate([world["S7"], R])
    pf8 = _write_pssm(tmp / "eight.pssm", names + ["r"], S8)
    r = _run(["-l", str(K), "--pssm", pf8, "--pssm-compare", "self", "--pssm-compare-threshold", "10",
              "--pssm-compare-overlap", "13", "-o", str(tmp / "cmp8.txt"), "--pssm-families-out", str(tmp / "fam8.txt")])
    assert r.returncode == 0, r.stdout + r.stderr
    h8 = capi.pssm_compare_host(capi.pssm_compare_columns(S8, "pearson"), 10.0, None, 13)
    assert (2, 7, 1) in zip(h8["x"].tolist(), h8["y"].tolist(), h8["d"].tolist()) and (3, 7, 0) in zip(
        h8["x"].tolist(), h8["y"].tolist(), h8["d"].tolist())
    lay8 = ref.layout(h8["x"], h8["y"], h8["d"], 8)
    assert lay8["n_conflicts"] >= 1 and "NOTE: %d hits contradict" % lay8["n_conflicts"] in r.stderr
    first = {}
    for m in lay8["order"]:
        first.setdefault(int(lay8["group"][m]), (names + ["r"])[m])
    assert open(str(tmp / "fam8.txt")).read() == "".join(
        "%s %s %d\n" % (first[int(lay8["group"][m])], (names + ["r"])[m], lay8["off"][m]) for m in lay8["order"])
    assert "w0 r 7\n" in open(str(tmp / "fam8.txt")).read()


def test_refusals(world):
    tmp = world["tmp"]
    out = tmp / "refused.txt"
    ok = ["-d", world["fa"], "-l", str(K), "--pssm", world["pf"], "--pssm-families", world["fam"], "-o", str(out)]

    def refused(args, *words):
        r = _run(args)
        assert r.returncode != 0 and "ERROR" in r.stderr, (args, r.stdout, r.stderr)
        for w in words:
            assert w in r.stderr, (w, r.stderr)
        assert not out.exists()

    def without(args, flag):
        i = args.index(flag)
        return args[:i] + args[i + 2:]

    def fam_file(name, lines):
        p = tmp / name
        p.write_text("".join(l + "\n" for l in lines))
        return str(p)

    good = ["%s %s %d" % l for l in world["fam_lines"]]
    refused(without(ok, "--pssm-families") + ["--pssm-families", fam_file("missing.txt", good[:-1])], "e2", "missing")
    refused(without(ok, "--pssm-families") + ["--pssm-families", fam_file("twice.txt", good + ["lone w0 4"])], "w0", "twice")
    refused(without(ok, "--pssm-families") + ["--pssm-families", fam_file("unknown.txt", good + ["lone zz 4"])], "zz")
    for bad in ("motif w0", "motif w0 x", "motif w0 -1", "motif w0 1 2", "motif w0 2147483648"):
        refused(without(ok, "--pssm-families") + ["--pssm-families", fam_file("bad.txt", [bad] + good[:2] + good[3:])],
                "bad.txt", "line 1")
    refused(without(ok, "--pssm-families") + ["--pssm-families", str(tmp / "nowhere.txt")], "nowhere.txt")
    for flag, value in (("--pssm-top", "3"), ("--pssm-per-sequence", "1"), ("--pssm-pvalue-column", "1"),
                        ("--pssm-refine", "2"), ("--pssm-rank", "5"), ("--pssm-pvalue", "0.01")):
        more = ["--pssm-out", str(tmp / "o.pssm")] if flag in ("--pssm-rank", "--pssm-refine", "--pssm-pvalue") else []
        refused(ok + [flag, value] + more, "--pssm-families", flag)
    refused(ok + ["--pssm-compare", "self", "--pssm-compare-threshold", "10"], "--pssm-families", "--pssm-compare")
    refused(without(ok, "--pssm-families") + ["--pssm-family-blocks", "2"], "--pssm-family-blocks", "--pssm-families")
    refused(without(ok, "--pssm-families") + ["--pssm-family-threshold", "2"], "--pssm-family-threshold", "--pssm-families")
    refused(without(ok, "--pssm") , "--pssm-families", "--pssm")
    for bad in ("0", "-1", "x", "1.5", ""):
        refused(ok + ["--pssm-family-blocks", bad], "--pssm-family-blocks")
    for bad in ("nan", "inf", "-inf", "x", ""):
        refused(ok + ["--pssm-family-threshold", bad], "--pssm-family-threshold")
    # --pssm-families-out belongs to --pssm-compare self
    refused(without(ok, "--pssm-families") + ["--pssm-families-out", str(tmp / "f.txt")], "--pssm-families-out")
    refused(["-l", str(K), "--pssm", world["pf"], "--pssm-compare", world["pf"], "--pssm-compare-threshold", "10", "-o",
             str(out), "--pssm-families-out", str(tmp / "f.txt")], "--pssm-families-out", "self")
    assert not (tmp / "f.txt").exists()
    # what --pssm refuses stays refused
    refused(ok + ["-c", world["pf"]], "--pssm", "-c")
    refused(ok + ["--topk", "3"], "--pssm", "--topk")
    refused(ok + ["--gpus", "2"], "--pssm", "--gpus")
    # a family of profiles the library refuses: 4097 lines cannot be written here, but an offset sum that breaks the
    # key width cannot either; a value the library refuses comes back with its text
    big = world["S7"].copy()
    big[0, 0, 0] = 3e30
    refused(without(ok, "--pssm") + ["--pssm", _write_pssm(tmp / "big.pssm", world["names"], big)], "2^100")
