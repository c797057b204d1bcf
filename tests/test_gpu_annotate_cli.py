"""hs_motif_both_points --best-per-position 1 (the annotation through the host programs): over a FASTA database
and over a points database, on one GPU, through the communicator with one rank, with two and three rank threads
on one GPU (every rank annotates its block of the centres, hs_merge_best merges) and under the table and bucket
partitions -- always the file the numpy rule (tests/annotate_ref.py) predicts from the plain run's hits."""
import subprocess

import numpy as np
import pytest

from tests import annotate_ref as ar
from tests.test_host_cli import _bin, _write_points

pytestmark = pytest.mark.gpu

_LETTERS = "ARNDCQEGHILKMFPSTWYV"


def _run(*args):
    r = subprocess.run([_bin(), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _hits_of_plain_run(k, K, L, W, R, planes_file, codes, centers, plain_file, names):
    """The hits the plain run wrote, with their tables and unrounded distances: the same search through the
    library with the run's planes -- checked to BE the plain run's file, line for line."""
    from hsearch_amd import Engine
    raw = np.fromfile(planes_file, dtype=np.float64)
    a = raw[:L * K * 8 * k].reshape(L, K, 8 * k)
    b = raw[L * K * 8 * k:].reshape(L, K)
    eng = Engine(k, K, L, W, a, b)
    eng.index_build(codes)
    hits = eng.query(centers, R)
    eng.close()
    text = "".join("p%d %s %g\n" % (q, names[i], d) for q, i, d in zip(hits["q"], hits["id"], hits["dist"]))
    assert open(plain_file).read() == text
    return hits


def _variants(tmp_path, common):
    outs = {}
    for tag, extra in (("one", ()), ("comm1", ("--gpus", "1")),
                       ("lb2", ("--gpus", "2", "--transport", "loopback")),
                       ("lb3", ("--gpus", "3", "--transport", "loopback")),
                       ("tables", ("--gpus", "2", "--transport", "loopback", "--partition", "tables")),
                       ("buckets", ("--gpus", "2", "--transport", "loopback", "--partition", "buckets"))):
        out = str(tmp_path / ("best_" + tag))
        _run(*common, "-o", out, "--best-per-position", "1", *extra)
        outs[tag] = open(out).read()
    return outs


def test_best_per_position_over_a_fasta_database(tmp_path, oracle):
    k, K, L, W, R, seed = 25, 2, 4, 150.0, 45.0, 33
    rng = np.random.default_rng(15)
    base = "".join(_LETTERS[i] for i in rng.integers(0, 20, size=60))
    seqs = []
    for _ in range(12):  # near-copies: windows with many suitors
        s_ = list(base)
        for _ in range(3):
            s_[rng.integers(0, len(s_))] = _LETTERS[rng.integers(0, 20)]
        seqs.append("".join(s_))
    fa = str(tmp_path / "db.fa")
    with open(fa, "w") as f:
        for i, s_ in enumerate(seqs):
            f.write(">p%d\n%s\n" % (i, s_))
    names, rows = [], []
    for i, s_ in enumerate(seqs):
        for j in range(len(s_) - k + 1):
            names.append("p%d#%d$%d@%s*%d" % (i, i, j, s_[j:j + k], len(names)))
            rows.append([_LETTERS.index(c) for c in s_[j:j + k]])
    codes = np.array(rows, dtype=np.uint8)
    pts = oracle.embed_codes(codes)
    pick = rng.choice(len(pts), 30, replace=False)
    centers = np.concatenate([pts[pick[:15]], pts[pick[15:]] + rng.normal(0, 0.3, size=(15, 8 * k)),
                              pts[pick[:15]]])  # exact ties between centres, in different query blocks
    cen, plain, planes = str(tmp_path / "cen"), str(tmp_path / "plain"), str(tmp_path / "planes")
    _write_points(cen, centers)
    common = ["-d", fa, "-c", cen, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R)]
    _run(*common, "-o", plain, "--seed", str(seed), "--planes-out", planes)
    hits = _hits_of_plain_run(k, K, L, W, R, planes, codes, centers, plain, names)
    best = ar.annotate(hits)
    assert len(best["id"]) > 100 and len(set(best["q"].tolist())) > 10 and ar.tie_levels(hits)[1] > 0
    want = "".join("%s p%d %g\n" % (names[i], q, d) for i, q, d in zip(best["id"], best["q"], best["dist"]))
    for tag, text in _variants(tmp_path, common + ["--planes", planes]).items():
        assert text == want, tag


def test_best_per_position_over_a_points_database(tmp_path):
    from hsearch_amd import synth
    k, K, L, W, R, seed = 15, 4, 4, 100.0, 30.0, 5
    codes = synth.make_db(3000, k, seed=11)
    qcodes, _ = synth.make_query_codes(codes, 90, seed=3)
    jittered, _ = synth.make_queries(codes, 60, jitter=0.25, seed=4)
    centers = np.concatenate([synth.embed(qcodes), jittered, synth.embed(qcodes[:30])])
    names = ["p%d" % i for i in range(len(codes))]
    db, cen, plain, planes = [str(tmp_path / n) for n in ("db", "cen", "plain", "planes")]
    _write_points(db, synth.embed(codes))
    _write_points(cen, centers)
    common = ["-d", db, "-c", cen, "-l", str(k), "-K", str(K), "-L", str(L), "-W", repr(W), "-T", repr(R)]
    _run(*common, "-o", plain, "--seed", str(seed), "--planes-out", planes)
    hits = _hits_of_plain_run(k, K, L, W, R, planes, codes, centers, plain, names)
    best = ar.annotate(hits)
    assert 0 < len(best["id"]) < len(hits["id"]) and ar.tie_levels(hits)[1] > 0
    want = "".join("%s p%d %g\n" % (names[i], q, d) for i, q, d in zip(best["id"], best["q"], best["dist"]))
    outs = _variants(tmp_path, common + ["--planes", planes])
    for tag, text in outs.items():
        assert text == want, tag
    # with extra probes the annotation follows the multi-probe hit list
    mp_plain, mp_best = str(tmp_path / "mp_plain"), str(tmp_path / "mp_best")
    _run(*common, "--planes", planes, "-o", mp_plain, "--probes", "3")
    _run(*common, "--planes", planes, "-o", mp_best, "--probes", "3", "--best-per-position", "1")
    reached = sorted(set(int(ln.split()[1][1:]) for ln in open(mp_plain)))
    got = [int(ln.split()[0][1:]) for ln in open(mp_best)]
    assert got == reached and len(reached) >= len(best["id"])
