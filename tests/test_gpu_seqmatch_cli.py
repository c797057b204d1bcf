"""`hs_motif_both_points --per-sequence 1` and `--query-fasta FILE` on the GPU, over a FASTA database of the proteins
tests/test_gpu_seqmatch.py searches: the written lines are parsed back and compared with the numpy rule
(tests/seqmatch_ref.py) applied to the list call of an engine with the program's planes -- distances bit for bit --,
plain and with --radii and -M; and the refused flag combinations."""
import subprocess

import numpy as np
import pytest

from hsearch_amd import Engine, capi
from tests import seqmatch_ref as sr
from tests.test_gpu_components_cli import _LETTERS, _planes_of_seed
from tests.test_host_cli import _bin

pytestmark = pytest.mark.gpu

_K, _SEED = sr.K_MER, 23


def _fasta(path, prefix, res, start):
    with open(path, "w") as f:
        for s, (a, b) in enumerate(zip(start[:-1], start[1:])):
            f.write(">%s%d some description\n%s\n" % (prefix, s, "".join(_LETTERS[c] for c in res[int(a):int(b)])))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seqmatch_cli")
    P = sr.make_proteins()
    lens = np.diff(P["db_start"].astype(np.int64))
    lens = lens[lens > 0]  # (a FASTA file cannot hold a protein without residues)
    db_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(db_start[-1]) == len(P["db"]) and (lens < _K).any() and (lens == _K).any()
    qry, qry_start = P["qry"], P["qry_start"]
    # one more protein that holds the first centre three times: a (centre, protein) row of several hits, lo < hi
    rng = np.random.default_rng(3)
    first = qry[:_K]
    rep = np.concatenate([first, rng.integers(0, 20, 4), first, rng.integers(0, 20, 9), first]).astype(np.uint8)
    db = np.concatenate([P["db"], rep])
    db_start = np.append(db_start, len(db)).astype(np.uint64)
    fa, qfa, cfa = (str(tmp / x) for x in ("db.fa", "query.fa", "centres.fa"))
    _fasta(fa, "db", db, db_start)
    _fasta(qfa, "qp", qry, qry_start)
    Q = capi.protein_queries(qry, qry_start, _K)
    pick = np.arange(0, len(Q["qcodes"]), 7)
    centres = Q["qcodes"][pick]
    names = ["c%d" % i for i in range(len(centres))]
    with open(cfa, "w") as f:
        for nm, row in zip(names, centres):
            f.write(">%s\n%s\n" % (nm, "".join(_LETTERS[c] for c in row)))
    a, b = _planes_of_seed(tmp, _K, sr.LSH["K"], sr.LSH["L"], sr.LSH["W"], _SEED)
    eng = Engine(_K, sr.LSH["K"], sr.LSH["L"], sr.LSH["W"], a, b)
    eng.index_build_windows(db, db_start)
    base = [_bin(), "-d", fa, "-l", str(_K), "-K", str(sr.LSH["K"]), "-L", str(sr.LSH["L"]), "-W", repr(sr.LSH["W"]),
            "--seed", str(_SEED)]
    yield dict(tmp=tmp, eng=eng, id_start=capi.window_id_start(db_start, _K), Q=Q, centres=centres, names=names,
               base=base, cfa=cfa, qfa=qfa, n_qp=len(qry_start) - 1)
    eng.close()


def _run(cmd, out):
    r = subprocess.run(cmd + ["-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return [ln.split(" ") for ln in open(out).read().splitlines()]


def _expected(rows, id_start, group_name, with_diag):
    out = []
    for i in range(len(rows["count"])):
        s = int(rows["seq"][i])
        line = [group_name(int(rows["group"][i])), "db%d#%d" % (s, s), str(int(rows["count"][i])),
                str(int(rows["best_id"][i]) - int(id_start[s])), float(rows["best_dist"][i]).hex(),
                str(int(rows["lo"][i])), str(int(rows["hi"][i]))]
        out.append(line + ([str(int(rows["diag"][i]))] if with_diag else []))
    return out


def _parsed(lines):
    return [ln[:4] + [float(ln[4]).hex()] + ln[5:] for ln in lines]  # (the printed distance reads back bit for bit)


def test_per_sequence_lines(world):
    w, eng = world, world["eng"]
    cmd = w["base"] + ["-c", w["cfa"], "--per-sequence", "1"]
    hits = eng.query_codes(w["centres"], sr.R)
    want = sr.seq_match(hits, w["id_start"], None, None)
    assert len(want["count"]) > 20 and want["count"].max() >= 3 and (want["hi"] > want["lo"]).any()
    got = _parsed(_run(cmd + ["-T", repr(sr.R)], str(w["tmp"] / "ps.txt")))
    assert got == _expected(want, w["id_start"], lambda g: w["names"][g], False)
    # every centre at its own radius, three extra probes per table
    rng = np.random.default_rng(6)
    radii = rng.choice(np.array([0.0, 8.0, 12.0, 20.0]), len(w["centres"]))
    rad = str(w["tmp"] / "radii")
    order = rng.permutation(len(radii))
    open(rad, "w").write("".join("%s %r\n" % (w["names"][i], float(radii[i])) for i in order))
    eng.set_multiprobe(3)
    try:
        hits = eng.query_radii(w["centres"], radii, codes=True)
    finally:
        eng.set_multiprobe(0)
    want = sr.seq_match(hits, w["id_start"], None, None)
    assert len(want["count"]) > 10
    got = _parsed(_run(cmd + ["--radii", rad, "-M", "3"], str(w["tmp"] / "ps_r.txt")))
    assert got == _expected(want, w["id_start"], lambda g: w["names"][g], False)


def test_query_fasta_lines(world):
    w, eng, Q = world, world["eng"], world["Q"]
    cmd = w["base"] + ["--query-fasta", w["qfa"]]
    name = lambda g: "qp%d#%d" % (g, g)
    hits = eng.query_codes(Q["qcodes"], sr.R)
    want = sr.seq_match(hits, w["id_start"], Q["q_group"], Q["q_off"])
    assert want["count"].max() >= 130 and (want["diag"] < 0).any() and (want["diag"] > 0).any()
    got = _parsed(_run(cmd + ["-T", repr(sr.R)], str(w["tmp"] / "qf.txt")))
    assert got == _expected(want, w["id_start"], name, True)
    # a radius per query protein (named by its whole '>' line), three extra probes
    per = np.array([12.0, 0.0, 20.0, 8.0, 12.0, 5.0, 12.0, 3.0])[:w["n_qp"]]
    rad = str(w["tmp"] / "radii_q")
    open(rad, "w").write("".join("qp%d some description %r\n" % (g, float(r)) for g, r in enumerate(per)))
    eng.set_multiprobe(3)
    try:
        hits = eng.query_radii(Q["qcodes"], per[Q["q_group"]], codes=True)
    finally:
        eng.set_multiprobe(0)
    want = sr.seq_match(hits, w["id_start"], Q["q_group"], Q["q_off"])
    assert len(want["count"]) > 10
    got = _parsed(_run(cmd + ["--radii", rad, "-M", "3"], str(w["tmp"] / "qf_r.txt")))
    assert got == _expected(want, w["id_start"], name, True)


def test_refused_combinations(world):
    w = world
    out = str(w["tmp"] / "never.txt")
    ps = w["base"] + ["-c", w["cfa"], "-T", "12", "-o", out, "--per-sequence", "1"]
    qf = w["base"] + ["--query-fasta", w["qfa"], "-T", "12", "-o", out]
    for cmd, word in ((ps + ["--gpus", "2"], "--gpus"), (ps + ["--topk", "3"], "--topk"),
                      (ps + ["--best-per-position", "1"], "--best-per-position"), (qf + ["--gpus", "2"], "--gpus"),
                      (qf + ["--topk", "3"], "--topk"), (qf + ["--best-per-position", "1"], "--best-per-position"),
                      (qf + ["-c", w["cfa"]], "-c")):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ERROR" in r.stderr and word in r.stderr, cmd
    import os
    assert not os.path.exists(out)
