"""`hs_motif_both_points -d proteins.fa -l k --pssm FILE --pssm-families FAM --pssm-family-shift G
[--pssm-family-gap-open X] [--pssm-family-gap-extend Y] [--pssm-family-blocks C] [--pssm-family-threshold T] -o OUT` on
the GPU: the bytes of OUT from the host rule (capi.pssm_family_chain_hits over tests/pssm_ref.py's scan) on the gapped
planted proteins, the unchanged bytes of the family rows without the new option, and every refused combination."""
import subprocess

import numpy as np
import pytest

from hsearch_amd import capi
from tests import pssm_chain_ref as ref, pssm_family_ref as fam, pssm_ref
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

K, A = 25, 20
INS = 2


def _run(args):
    return subprocess.run([_bin()] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The gapped planted proteins (two residues inserted in proteins 1, 6, 8, 9) as FASTA, the motif's three window
    profiles and four unrelated ones in a shuffled file order, and a FAM file with every family's lines in offset
    order, the families interleaved."""
    tmp = tmp_path_factory.mktemp("pssm_chain_cli")
    c = ref.planted_gapped(ins=INS)
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
    t = np.array([np.sort(sc[m])[-200] if n[0] == "e" else fam.PLANTED_T for m, n in enumerate(names)])
    pf = tmp / "prof.pssm"
    with open(str(pf), "w") as f:
        for n, prof, tt in zip(names, S, t):
            f.write(">%s %.17g\n" % (n, tt))
            for row in prof:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    fam_lines = [("other", "e2", 0), ("motif", "w0", 0), ("other", "e3", 2), ("motif", "w3", 3), ("lone", "e0", 0),
                 ("other", "e1", 2), ("motif", "w6", 6)]
    fam_file = tmp / "fam.txt"
    fam_file.write_text("".join("%s %s %d\n" % l for l in fam_lines) + "\n")
    return dict(c, tmp=tmp, fa=str(fa), pf=str(pf), fam=str(fam_file), fam_lines=fam_lines, S7=S, t7=t, names=names)


def _ordered(world):
    """the CLI's own ordering by (family in order of first appearance, offset, file order)"""
    names = world["names"]
    fam_of = {n: f for f, n, _ in world["fam_lines"]}
    off_of = {n: o for _, n, o in world["fam_lines"]}
    fams = []
    for f, _, _ in world["fam_lines"]:
        if f not in fams:
            fams.append(f)
    order = sorted(range(len(names)), key=lambda m: (fams.index(fam_of[names[m]]), off_of[names[m]], m))
    m_group = np.array([fams.index(fam_of[names[m]]) for m in order], dtype=np.uint32)
    m_off = np.array([off_of[names[m]] for m in order], dtype=np.uint32)
    hits = pssm_ref.scan(world["S7"][order], world["t7"][order], world["codes"])
    return fams, order, m_group, m_off, hits


def _expected(world, shift, gap_open=0.0, gap_ext=0.0, blocks=1, threshold=None):
    fams, order, m_group, m_off, hits = _ordered(world)
    names = world["names"]
    rows = capi.pssm_family_chain_hits(hits["m"], hits["id"], hits["score"], len(order), world["id_start"], m_group,
                                       m_off, shift, gap_open, gap_ext, min_count=blocks,
                                       t_group=None if threshold is None else np.full(len(fams), threshold))
    ids = world["id_start"].astype(np.int64)
    lines = []
    for r in range(len(rows["group"])):
        s = int(rows["seq"][r])
        lines.append("%s p%d#%d %d %d %.17g %s %d %s %d %d\n" % (
            fams[rows["group"][r]], s, s, rows["count"][r], rows["gaps"][r], rows["score"][r],
            names[order[rows["first_m"][r]]], int(rows["first_id"][r]) - ids[s], names[order[rows["last_m"][r]]],
            int(rows["last_id"][r]) - ids[s], rows["shift"][r]))
    return "".join(lines), rows, fams


@pytest.mark.parametrize("shift,gap_open,gap_ext,blocks,threshold",
                         [(3, 4.0, 1.0, 3, None), (3, None, None, None, None), (0, 4.0, None, 2, None),
                          (1, None, 0.5, 3, None), (65535, 0.1, 2.0 ** -20, 2, 100.0)])
def test_output_equals_host_rule(world, shift, gap_open, gap_ext, blocks, threshold):
    out = str(world["tmp"] / ("out_%s_%s_%s_%s.txt" % (shift, gap_open, blocks, threshold)))
    cmd = ["-d", world["fa"], "-l", str(K), "--pssm", world["pf"], "--pssm-families", world["fam"], "-o", out,
           "--pssm-family-shift", str(shift)]
    for flag, v in (("--pssm-family-gap-open", gap_open), ("--pssm-family-gap-extend", gap_ext),
                    ("--pssm-family-threshold", threshold)):
        if v is not None:
            cmd += [flag, "%.17g" % v]
    if blocks is not None:
        cmd += ["--pssm-family-blocks", str(blocks)]
    r = _run(cmd)
    assert r.returncode == 0, r.stdout + r.stderr
    want, rows, fams = _expected(world, shift, gap_open or 0.0, gap_ext or 0.0, blocks or 1, threshold)
    assert open(out).read() == want
    assert "number of rows %d" % len(rows["group"]) in r.stdout and "in 3 families" in r.stdout
    motif = rows["group"] == fams.index("motif")
    if blocks == 3:       # three blocks of the motif family (random profiles at loose thresholds chain by chance too)
        found = dict(zip(rows["seq"][motif].tolist(), rows["shift"][motif].tolist()))
        if shift >= INS:  # all nine planted proteins, the four gapped ones at the insertion's length
            assert found == {s: (INS if s in ref.PLANTED_GAPPED else 0) for s in world["planted"]}
        else:
            assert sorted(found) == list(ref.PLANTED_UNGAPPED)
    assert len(want.splitlines()) >= 5


def test_without_the_option_the_bytes_are_the_family_rows(world):
    """--pssm-families without --pssm-family-shift writes what the family rule gives, as before the option existed."""
    out = str(world["tmp"] / "rows.txt")
    r = _run(["-d", world["fa"], "-l", str(K), "--pssm", world["pf"], "--pssm-families", world["fam"], "-o", out,
              "--pssm-family-blocks", "2"])
    assert r.returncode == 0, r.stdout + r.stderr
    fams, order, m_group, m_off, hits = _ordered(world)
    rows = capi.pssm_family_hits(hits["m"], hits["id"], hits["score"], len(order), world["id_start"], m_group=m_group,
                                 m_off=m_off, min_count=2)
    ids = world["id_start"].astype(np.int64)
    names = world["names"]
    want = "".join("%s p%d#%d %d %d %.17g %s %d %.17g %d %d\n" % (
        fams[rows["group"][i]], s, s, rows["diag"][i], rows["count"][i], rows["sum"][i],
        names[order[rows["best_m"][i]]], int(rows["best_id"][i]) - ids[s], rows["best_score"][i], rows["lo"][i],
        rows["hi"][i]) for i, s in enumerate(rows["seq"].tolist()))
    assert open(out).read() == want and len(want.splitlines()) >= 5


def test_refusals(world):
    tmp = world["tmp"]
    out = tmp / "refused.txt"
    ok = ["-d", world["fa"], "-l", str(K), "--pssm", world["pf"], "--pssm-families", world["fam"], "-o", str(out)]
    chain = ok + ["--pssm-family-shift", "3"]

    def refused(args, *words):
        r = _run(args)
        assert r.returncode != 0 and "ERROR" in r.stderr, (args, r.stdout, r.stderr)
        for w in words:
            assert w in r.stderr, (w, r.stderr)
        assert not out.exists()

    def without(args, flag):
        i = args.index(flag)
        return args[:i] + args[i + 2:]

    # the gap options without the shift; the shift without the families
    refused(ok + ["--pssm-family-gap-open", "1"], "--pssm-family-gap-open", "--pssm-family-shift")
    refused(ok + ["--pssm-family-gap-extend", "1"], "--pssm-family-gap-extend", "--pssm-family-shift")
    refused(without(chain, "--pssm-families"), "--pssm-family-shift", "--pssm-families")
    for bad in ("-1", "65536", "x", "1.5", "", "+3", "3x"):
        refused(ok + ["--pssm-family-shift", bad], "--pssm-family-shift", "65535")
    for flag in ("--pssm-family-gap-open", "--pssm-family-gap-extend"):
        for bad in ("-1", "-1e-300", "nan", "inf", "x", "", "1x"):
            refused(chain + [flag, bad], flag)
    # a FAM whose offsets decrease inside a family, in line order: the family rows take it, the chain does not
    lines = ["%s %s %d" % l for l in world["fam_lines"]]
    swapped = tmp / "swapped.txt"
    swapped.write_text("".join(l + "\n" for l in [lines[3], lines[1]] + lines[:1] + lines[2:3] + lines[4:]))
    refused(without(chain, "--pssm-families") + ["--pssm-families", str(swapped)], "swapped.txt", "line 2", "motif",
            "--pssm-families-out")
    r = _run(without(ok, "--pssm-families") + ["--pssm-families", str(swapped)])
    assert r.returncode == 0 and out.exists()
    out.unlink()
    # what --pssm-families refuses stays refused beside the new option
    refused(chain + ["--pssm-family-blocks", "0"], "--pssm-family-blocks")
    refused(chain + ["--pssm-family-threshold", "nan"], "--pssm-family-threshold")
    refused(chain + ["--pssm-top", "3"], "--pssm-families", "--pssm-top")
    refused(chain + ["--gpus", "2"], "--pssm", "--gpus")
