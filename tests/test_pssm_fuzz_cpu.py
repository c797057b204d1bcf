"""The host rules of the profile calls on the random worlds of tests/pssm_fuzz_cases.py, without a GPU: every rule over
the world's reference hits -- shuffled, a fifth of them twice -- against the Python references of tests/*_ref.py, every
array bit for bit; the p-values also against the exact probability where the k-mers can be enumerated.  The last two
tests pin what the default case set reaches (on the references alone, so that the GPU test over the same worlds cannot
pass by being vacuous) and show that a mutated rule breaks several worlds."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from hsearch_amd import capi

import pssm_chain_ref
import pssm_compare_ref
import pssm_counts_ref
import pssm_family_ref
import pssm_fuzz_cases as cases
import pssm_null_ref
import pssm_seq_ref
import pssm_topk_ref
import pssm_weights_ref

SEEDS = range(cases.DEFAULT_CASES)
_DONE = {}


def _world(seed):
    """dict(w: the world, want: its references): computed once per seed"""
    if seed not in _DONE:
        w = cases.world(seed)
        _DONE[seed] = dict(w=w, want=cases.references(w))
    return _DONE[seed]


def _shuffled(w):
    h = w["hits"]
    rng = np.random.default_rng(w["seed"])
    n = len(h["m"])
    p = rng.permutation(np.concatenate([np.arange(n), rng.integers(0, max(n, 1), size=n // 5)]).astype(np.int64))
    return h["m"][p], h["id"][p], h["score"][p]


def _host_chain(w, hits):
    args, kw = cases.chain_args(w)
    return capi.pssm_family_chain_hits(*hits, w["nm"], w["id_start"], *args, want_path=True, **kw)


def _host_family(w, hits):
    return capi.pssm_family_hits(*hits, w["nm"], w["id_start"], **cases.family_args(w))


def _same_compare(got, want, what):
    for f in ("x", "y", "d", "cnt"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f)
    assert pssm_compare_ref.same_bits(got["score"], want["score"]), what


def _exact_bracket(w, S, m):
    """p_lo <= P{score >= t} <= p_hi in exact rational arithmetic, at every attained score of profile m and between
    them (tests/test_pssm_null_cpu.py's invariant), where the A^k k-mers can be enumerated"""
    k, A, bg = w["k"], w["A"], w["bg"]
    mass = [Fraction(float(b)) for b in bg]
    km = []
    for x in itertools.product(range(A), repeat=k):
        s, p = 0.0, Fraction(1)
        for pos in range(k):
            s = s + float(S[pos][x[pos]])
            p *= mass[x[pos]]
        km.append((s, p))
    at_least, total = {}, Fraction(0)                     # score -> the exact mass of the k-mers at or above it
    for s, p in sorted(km, reverse=True):
        total += p
        at_least[s] = total
    sc = sorted(at_least)
    mids = [a / 2 + b / 2 for a, b in zip(sc, sc[1:])]
    ts = np.array(sc + mids)
    exact = [at_least[s] for s in sc] + [at_least[b if t > a else a] for a, b, t in zip(sc, sc[1:], mids)]
    pv = capi.pssm_pvalue_host(S[None], bg, np.zeros(len(ts), np.uint32), ts, w["t_lo"], w["bins"])
    for t, P, hi, lo in zip(ts, exact, pv["p_hi"], pv["p_lo"]):
        assert Fraction(float(lo)) <= P <= Fraction(float(hi)), (w["seed"], m, t, float(P), lo, hi)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_rules_equal_the_references(seed):
    w, want = _world(seed)["w"], _world(seed)["want"]
    nm, ids, A = w["nm"], w["id_start"], w["A"]
    hits = _shuffled(w)
    what = (seed, w["style"], w["k"], A, nm, w["n"])
    pssm_seq_ref.same_rows(capi.pssm_seq_hits(*hits, nm, ids), want["seq"], what)
    pssm_family_ref.same_rows(capi.pssm_family_hits(*hits, nm, ids), want["fam_plain"], what)
    pssm_family_ref.same_rows(_host_family(w, hits), want["fam"], what)
    pssm_chain_ref.same_chains(_host_chain(w, hits), want["chain"], what)
    pssm_topk_ref.same_rows(capi.pssm_topk_hits(*hits, nm, w["topk"]), want["topk_hits"], what)
    pssm_counts_ref.same_counts(capi.pssm_count_hits(w["codes"], A, *hits, nm), want["counts"], what)
    pssm_counts_ref.same_counts(capi.pssm_count_hits(w["codes"], A, *hits, nm, ids), want["counts_seq"], what)
    pssm_weights_ref.same_weights(capi.pssm_weight_hits(w["codes"], A, *hits, nm), want["weights"], what)
    pssm_weights_ref.same_weights(capi.pssm_weight_hits(w["codes"], A, *hits, nm, ids), want["weights_seq"], what)
    X, Y = cases.compare_args(w)
    _same_compare(capi.pssm_compare_host(w["S"], w["cmp_t"], None, w["min_overlap"]), want["cmp_self"], what)
    _same_compare(capi.pssm_compare_host(X, w["cmp_t"], Y, w["min_overlap"]), want["cmp_xy"], what)
    # the null model: the p-values of the hits in another order, the thresholds, and the bracket
    order = np.random.default_rng(seed).permutation(len(want["pv_m"]))
    pv = capi.pssm_pvalue_host(w["S"], w["bg"], want["pv_m"][order], want["pv_score"][order], w["t_lo"], w["bins"])
    assert pssm_null_ref.same_bits(pv["p_hi"], want["p_hi"][order]), what
    assert pssm_null_ref.same_bits(pv["p_lo"], want["p_lo"][order]), what
    assert np.all(pv["p_lo"] <= pv["p_hi"]) and np.all(pv["p_lo"] >= 0.0)
    th = capi.pssm_threshold_host(w["S"], w["bg"], w["p"], w["t_lo"], w["bins"])
    for f in ("t", "p_hi", "p_lo"):
        assert pssm_null_ref.same_bits(th[f], want["thr"][f]), (what, f)
    assert np.array_equal(th["flag"], want["thr"]["flag"]) and np.all(th["p_lo"] <= th["p_hi"]), what
    if A ** w["k"] <= 1024:
        for m in range(min(nm, 3)):
            _exact_bracket(w, w["S"][m], m)


def test_the_case_set_reaches_the_edges():
    """Over the default seeds, on the references alone: cases.FLOORS worlds at least reach every edge.  (A generator
    that misses one is changed, not the floor.)"""
    total = dict.fromkeys(cases.FLOORS, 0)
    seconds = 0.0
    for seed in SEEDS:
        d = _world(seed)
        seconds = max(seconds, d["want"]["seconds"])
        for name, yes in d["want"]["reached"].items():
            total[name] += bool(yes)
    print("worlds that reach each edge:", total, " the references' largest CPU time per world: %.2f s" % seconds)
    for name, floor in cases.FLOORS.items():
        assert total[name] >= floor, (name, total[name], floor)
    # "a few seconds" of CPU time per world at the most: a generator that outgrows it gets tighter bounds, not fewer cases
    assert seconds < 5.0, seconds
    for w in (_world(s)["w"] for s in SEEDS):
        assert len(w["hits"]["m"]) <= cases.MAX_HITS
        assert cases.segment_sizes(w["sc"] >= w["t"][:, None], w["m_group"], w["id_start"]).max() <= cases.MAX_SEGMENT


def test_a_mutated_rule_breaks_several_worlds():
    """The chain's tie order flipped (pssm_chain_ref's pred_m_ascending) and a family row summed in reverse
    (pssm_family_ref's reverse_sum): each mutant disagrees with the host rule in several worlds, so a device with either
    mistake fails several cases of the GPU test."""
    chain_broken, sum_broken = [], []
    for seed in SEEDS:
        w = _world(seed)["w"]
        h, hits = w["hits"], (w["hits"]["m"], w["hits"]["id"], w["hits"]["score"])
        args, kw = cases.chain_args(w)
        mutant = pssm_chain_ref.chains(h, w["nm"], w["id_start"], *args, pred_m_ascending=True, **kw)
        try:
            pssm_chain_ref.same_chains(_host_chain(w, hits), mutant, seed)
        except AssertionError:
            chain_broken.append(seed)
        mutant = pssm_family_ref.rows(h, w["nm"], w["id_start"], reverse_sum=True, **cases.family_args(w))
        try:
            pssm_family_ref.same_rows(_host_family(w, hits), mutant, seed)
        except AssertionError:
            sum_broken.append(seed)
    print("worlds a flipped tie order breaks:", chain_broken, " worlds a reversed sum breaks:", sum_broken)
    assert len(chain_broken) >= 3 and len(sum_broken) >= 3, (chain_broken, sum_broken)
