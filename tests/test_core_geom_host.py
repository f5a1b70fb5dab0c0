"""The launch decisions and LDS layouts of the core modem's receive kernels over every geometry ofdm_create accepts:
tools/core_geom_check.cpp (the headers' own functions, checked in a program of its own) and its `--table` against the
class functions of core_sweep_cases.py (filter_F, sync_class, front_eligible, demod_class), which the sweep labels its cases
with.  Nothing is restated here: the headers are one side, the cases module the other."""
import os
import subprocess

import pytest

import core_sweep_cases as cs
from ofdm_uhd_amd import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("k_chan_filter", "k_sync", "k_front", "k_sync_exact", "k_sync_exact_wave", "k_rx_demod")
# the launches that pass their LDS size without raising the limit first (engine_rx.inc)
PLAIN_LAUNCH = ("k_chan_filter", "k_sync_exact_wave")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """Built without sanitizers (the header comment of the program gives the flags a sanitizer run adds)."""
    exe = str(tmp_path_factory.mktemp("geom") / "core_geom_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-Wno-unused-value", "-I",
                           os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "core_geom_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def table(checker):
    out = subprocess.check_output([checker, "--table"]).decode().splitlines()
    assert out[-1] == "core_geom_check ok"
    return [line.split() for line in out]


def _kv(fields):
    return {k: int(v) for k, v in (f.split("=") for f in fields)}


def test_every_accepted_geometry_passes_the_checker(checker):
    out = subprocess.check_output([checker]).decode().splitlines()
    assert out[-1] == "core_geom_check ok"
    lds = {l.split()[1]: int(l.split()[2]) for l in out if l.startswith("lds ")}
    assert set(lds) == set(KERNELS)
    for name, size in lds.items():
        assert 0 < size <= (64 * 1024 if name in PLAIN_LAUNCH else cs.LDS_CU), name
    print("largest dynamic LDS per kernel: %s" % ", ".join("%s %d" % kv for kv in sorted(lds.items())))
    # no geometry is one launch_demod refuses by itself: the refusal test_gpu_slicer.LDS_ERROR names needs the knob
    assert [l for l in out if l.startswith("refused k_rx_demod")][0].split()[2] == "0"


def test_filter_classes(table):
    runs = [(int(f[1]), int(f[2]), _kv(f[3:])) for f in table if f[0] == "filter"]
    assert [r[0] for r in runs] == [1, 33, 65, 129, 257] and runs[-1][1] == 512
    for lo, hi, kv in runs:
        for nt in (lo, hi):
            assert cs.filter_F(nt) == kv["F"], nt
        assert kv["Bmax"] == kv["F"] - lo + 1 and kv["Bmin"] == kv["F"] - hi + 1
        assert cs.filter_bpr(kv["F"]) * (kv["F"] // 8) == 256
    # the band of occupied_tones that gives each transform length from options: the design rule, not the table
    for N in cs.NS:
        for occ in cs.accepted_occ(N):
            assert cs.options_ntaps(N, occ) == len(config.channel_filter_taps(N, occ)) <= 512


def test_sync_classes(table):
    runs = [(int(f[1]), int(f[2]), int(f[3]), _kv(f[4:])) for f in table if f[0] == "sync"]
    assert sorted({r[0] for r in runs}) == list(cs.NS)
    for N in cs.NS:
        mine = [r for r in runs if r[0] == N]
        assert mine[0][1] == 1 and mine[-1][2] == N and all(a[2] + 1 == b[1] for a, b in zip(mine, mine[1:]))
        for _, lo, hi, kv in mine:
            for cp in (lo, hi):                      # both ends of every run: both sides of every boundary
                assert cs.sync_class(N, cp) == kv, (N, cp)
        # the sweep holds both sides of every boundary below the refusal
        cps = {c["CP"] for c in cs.CASES if c["N"] == N}
        for a, b in zip(mine, mine[1:]):
            if not b[3]["refused"]:
                assert {a[2], b[1]} <= cps, (N, a[2])


def test_front_classes(table):
    runs = [f for f in table if f[0] == "front"]
    seen = set()
    for f in runs:
        N, lo, hi, F = int(f[1]), int(f[2]), int(f[3]), _kv(f[4:5])["F"]
        spans = [] if f[6] == "none" else [tuple(int(v) for v in s.split("-")) for s in f[6:]]
        for nt in (lo, hi):
            assert cs.filter_F(nt) == F
            inside = set()
            for a, b in spans:
                inside |= {a, b}
                assert cs.front_eligible(N, a, nt) and cs.front_eligible(N, b, nt), (N, nt, a, b)
                if b < N:
                    assert not cs.front_eligible(N, b + 1, nt), (N, nt, b)
            if not spans:
                assert not any(cs.front_eligible(N, cp, nt) for cp in (1, N // 4, N)), (N, nt)
        seen.add(N)
    assert seen == set(cs.NS)
    for c in cs.CASES:                               # the label the GPU test picks its fused-front cases by
        nt = cs.case_ntaps(c)
        row = [f for f in runs if int(f[1]) == c["N"] and int(f[2]) <= nt <= int(f[3])][0]
        want = any(int(s.split("-")[0]) <= c["CP"] <= int(s.split("-")[1]) for s in row[6:] if s != "none")
        assert ("front" in cs.labels(c)) == want, c["name"]


def test_demod_classes(table):
    runs = [f for f in table if f[0] == "demod"]
    for f in runs:
        N, kv, lo, hi, cls = int(f[1]), _kv(f[2:6]), int(f[6]), int(f[7]), _kv(f[8:])
        for occ in (lo, hi):
            assert cs.demod_class(N, occ, kv["arity"], kv["shift"], bool(kv["grid"]), bool(kv["csi"])) == cls, (N, kv, occ)
    # from N = 2048 on the formulas alone reach all four settings inside the accepted band of the built-in map
    for N in (2048, 4096):
        got = {(_kv(f[8:])["twl"], _kv(f[8:])["smap"]) for f in runs if int(f[1]) == N and f[5] == "csi=0"
               and int(f[7]) >= cs.accepted_occ(N)[0] and int(f[6]) <= cs.accepted_occ(N)[-1]}
        assert got == {(1, 1), (1, 0), (0, 1), (0, 0)}, N
