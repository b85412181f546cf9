"""amg_partition_modularity (the host modularity partitioner) against the
independent restatement in tests/modularity_restated.py -- agg_of, naggs, rounds,
improvement passes and swaps, exactly -- with the invariants of every partition; the
C ABI's argument errors; the process-wide partitioner policy; symbols declared,
exported and bound.  No GPU.  The device path: tests/test_gpu_partition.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import modularity_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_partitioner_config_default", "amg_partition_modularity", "amg_partition_modularity_device",
       "amg_set_sa_partitioner", "amg_get_sa_partitioner")
OK, INVALID = 0, 1


def fa():
    import faer_amg_amd
    return faer_amg_amd


def check_invariants(agg, naggs, n, cf, stalled):
    agg = np.asarray(agg)
    assert agg.shape == (n,) and agg.min() == 0 and agg.max() == naggs - 1  # every node assigned
    first = np.full(naggs, n, np.int64)
    np.minimum.at(first, agg, np.arange(n))
    assert (first < n).all() and (np.diff(first) > 0).all()  # numbered by smallest node
    if not stalled:
        assert math.floor(n / cf) - 2 <= naggs <= n / cf


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_host_partitioner_equals_the_restatement(name):
    rows, cfg, want = R.case(name)
    n = len(rows)
    agg, na, info = fa().partition_modularity(R.to_scipy(rows), **cfg)
    assert na == want["naggs"]
    assert info["rounds"] == want["rounds"]
    assert info["improvement_passes"] == want["improvement_passes"]
    assert info["swaps"] == want["swaps"]
    assert agg.tolist() == want["agg_of"]
    assert info["passes"] == 0 and info["max_passes_in_round"] == 0 and not info["fallback"]
    sizes = np.bincount(agg, minlength=na)
    assert info["min_agg"] == sizes.min() and info["max_agg"] == sizes.max()
    check_invariants(agg, na, n, cfg.get("coarsening_factor", 8.0), want["stalled"])


def test_restatement_pass_form_is_the_serial_sweep():
    """The locally dominant passes give the serial sweep's pairs in every round (asserted
    inside), in a handful of passes with the mix tie-break."""
    got = R.partition(R.grid_rows(8, 8, 8), check_passes=True)
    assert got["rounds"] == len(got["pass_counts"]) >= 3  # 8 = 2^3, and the cut leaves a remainder
    assert max(got["pass_counts"]) <= 12
    assert got["naggs"] == 62  # 8^3 / 8 - 2: the T + 1 cut


def test_cases_cover_what_they_claim():
    # cf 2: the last round is cut at T + 1 pairs (a greedy matching is maximal, not perfect,
    # so a first full round leaves more than n / 2 vertices and a short second one follows)
    assert R.case("grid12_cf2")[2]["rounds"] in (1, 2)
    assert R.case("grid12_cf2")[2]["naggs"] in (862, 863, 864)
    assert R.case("isolated")[2]["stalled"] and R.case("two_nodes")[2]["stalled"]
    assert R.case("two_nodes")[2]["agg_of"] == [0, 0]
    assert not R.case("grid16_cf128")[2]["stalled"]
    assert R.case("grid16_cf128")[2]["naggs"] in (30, 31, 32)
    assert any(R.case(k)[2]["swaps"] > 0 for k in R.CASES)  # the improvement passes are exercised


def test_partitioner_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    for name in ("PartitionerConfig", "partition_modularity", "partition_modularity_device", "set_sa_partitioner",
                 "get_sa_partitioner"):
        assert callable(getattr(fa(), name)), name


def test_partitioner_config_default_and_layout():
    F = fa()
    c = F.PartitionerConfig()
    assert C.sizeof(c) == 32
    assert (c.coarsening_factor, c.agg_size_penalty, c.max_improvement_iters, c.max_passes) == (8.0, 1.0, 100, 0)
    assert F.lib().amg_partitioner_config_default(None) == INVALID
    assert C.sizeof(F.SaConfig()) == 64  # the policy is process-wide: amg_sa_config keeps its layout


def test_sa_partitioner_policy_default_and_range():
    F = fa()
    L = F.lib()
    v = C.c_int32(-7)
    assert L.amg_get_sa_partitioner(C.byref(v), None) == OK and v.value == 0  # MIS, by default
    kind, cfg = F.get_sa_partitioner()
    assert kind == 0 and cfg.coarsening_factor == 8.0
    assert L.amg_get_sa_partitioner(None, None) == INVALID
    assert b"null output" in L.amg_last_error()
    try:
        for bad in (2, -1):
            assert L.amg_set_sa_partitioner(bad, None) == INVALID
            assert b"partitioner must be 0" in L.amg_last_error()
            assert F.get_sa_partitioner()[0] == 0  # a refused value changes nothing
        badcfg = F.PartitionerConfig(coarsening_factor=0.5)
        assert L.amg_set_sa_partitioner(1, C.byref(badcfg)) == INVALID
        assert F.get_sa_partitioner()[0] == 0
        F.set_sa_partitioner("modularity", coarsening_factor=128.0, agg_size_penalty=0.5)
        kind, cfg = F.get_sa_partitioner()
        assert kind == 1 and cfg.coarsening_factor == 128.0 and cfg.agg_size_penalty == 0.5
        assert L.amg_set_sa_partitioner(1, None) == OK  # NULL: the defaults
        assert F.get_sa_partitioner()[1].coarsening_factor == 8.0
        F.set_sa_partitioner("mis")
        assert F.get_sa_partitioner()[0] == 0
    finally:
        assert L.amg_set_sa_partitioner(0, None) == OK
    assert F.get_sa_partitioner()[0] == 0


def test_partitioner_arguments_rejected_without_a_device():
    F = fa()
    L = F.lib()
    G = F.HostCsr(F._host_csr_from_scipy(R.to_scipy(R.path_rows(4))))
    rect = F.HostCsr(F._host_csr_from_scipy(R.to_scipy(R.path_rows(4))[:3, :]))
    cfg = F.PartitionerConfig()
    agg = np.full(4, -3, np.int64)
    info = np.full(8, -3, np.int64)
    na = C.c_int64(-3)
    pagg, pinfo = agg.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    for fn, g in ((L.amg_partition_modularity, G.h), (L.amg_partition_modularity_device, None)):
        assert fn(g, C.byref(cfg), None, C.byref(na), pinfo) == INVALID
        assert b"null output" in L.amg_last_error()
        assert fn(g, C.byref(cfg), pagg, None, pinfo) == INVALID
        assert b"null output" in L.amg_last_error()
        assert fn(g, None, pagg, C.byref(na), pinfo) == INVALID
        assert b"null partitioner config" in L.amg_last_error()
        for bad, msg in ((dict(coarsening_factor=0.99), b"coarsening_factor"),
                         (dict(coarsening_factor=float("nan")), b"coarsening_factor"),
                         (dict(agg_size_penalty=-1e-9), b"agg_size_penalty"),
                         (dict(max_passes=-1), b"negative")):
            c = F.PartitionerConfig(**bad)
            assert fn(g, C.byref(c), pagg, C.byref(na), pinfo) == INVALID
            assert msg in L.amg_last_error()
    # the config is looked at before the device handle: a null handle comes last
    assert L.amg_partition_modularity_device(None, C.byref(cfg), pagg, C.byref(na), pinfo) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_partition_modularity(None, C.byref(cfg), pagg, C.byref(na), pinfo) == INVALID
    assert L.amg_partition_modularity(rect.h, C.byref(cfg), pagg, C.byref(na), pinfo) == INVALID
    assert b"square" in L.amg_last_error()
    assert (agg == -3).all() and (info == -3).all() and na.value == -3
    assert L.amg_partition_modularity(G.h, C.byref(cfg), pagg, C.byref(na), None) == OK  # info8 is optional
    assert na.value == 1 and (agg == 0).all()


def test_zero_total_and_non_finite_strengths_are_invalid():
    F = fa()
    import scipy.sparse as sp
    empty = sp.csr_matrix((3, 3))
    with pytest.raises(F.AmgError, match="sum to zero"):
        F.partition_modularity(empty)
    rows = R.path_rows(4)
    rows[1][0] = (0, float("inf"))
    with pytest.raises(F.AmgError, match="not finite"):
        F.partition_modularity(R.to_scipy(rows))
    rows[1][0] = (1, 1.0)  # a self loop
    with pytest.raises(F.AmgError, match="no self loops"):
        F.partition_modularity(R.to_scipy(rows))
