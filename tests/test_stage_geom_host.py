"""The host geometry of the ten wideband stream stages over every shape they accept: tools/stage_geom_check.cpp (the
headers' own functions, checked in a program of its own) and its `--table` against the restatements the tests size their
streams with (tile_outputs, tile_inputs, history of tests/*_cases.py, through stage_harness.STAGES).  Nothing is restated
here: the headers are one side, the cases modules the other."""
import os
import subprocess

import pytest

import ddc_bank_cases
import ddc_cases
import duc_bank_cases
import duc_cases
import pfb_cases
import stage_harness as sh
import stage_sweep_cases as sw

ROOT = sh.ROOT
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_DEFAULT, LDS_DEVICE = 64 * 1024, 160 * 1024
# the stages whose launch passes its LDS size without raising the limit first
PLAIN_LAUNCH = ("ddc", "duc", "duc_bank", "pfb_synth", "pfb")
TILE_OUTPUTS = {"ddc": ddc_cases.tile_outputs, "ddc_bank": ddc_bank_cases.tile_outputs, "pfb": pfb_cases.tile_outputs,
                "duc": duc_cases.tile_outputs, "duc_bank": duc_bank_cases.tile_outputs}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """Built without sanitizers (the header comment of the program gives the flags a sanitizer run adds)."""
    exe = str(tmp_path_factory.mktemp("geom") / "stage_geom_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-Wno-unused-value", "-I",
                           os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "stage_geom_check.cpp")])
    return exe


def test_every_accepted_shape_passes_the_checker(checker):
    out = subprocess.check_output([checker]).decode().splitlines()
    assert out[-1] == "stage_geom_check ok"
    lds = {l.split()[1]: int(l.split()[2]) for l in out if l.startswith("lds ")}
    assert set(lds) == set(sh.STAGES)
    for name, size in lds.items():
        assert 0 < size <= (LDS_DEFAULT if name in PLAIN_LAUNCH else LDS_DEVICE), name
    print("largest dynamic LDS per stage: %s" % ", ".join("%s %d" % kv for kv in sorted(lds.items())))


def test_the_cases_modules_restate_the_headers_geometry(checker):
    out = subprocess.check_output([checker, "--table"]).decode().splitlines()
    assert out[-1] == "stage_geom_check ok"
    tiles, hists = {}, {}
    for line in out:
        f = line.split()
        if f[0] == "tile":
            shape = tuple(int(v) for v in f[2:-2])
            tiles[f[1], shape] = (int(f[-2].split("=")[1]), int(f[-1].split("=")[1]))
        elif f[0] == "hist":
            for nt in range(int(f[3]), int(f[4]) + 1):
                hists[f[1], int(f[2]), nt] = int(f[5])
    for name, st in sh.STAGES.items():
        two = name in ("resamp", "resamp_bank", "tx_resamp", "tx_resamp_bank")
        dims = sw._PFB_M if name in ("pfb", "pfb_synth") else range(1, 65)
        shapes = [(a, b) for a in dims for b in dims] if two else [(a,) for a in dims]
        assert {s for n, s in tiles if n == name} == set(shapes), name
        for shape in shapes:
            outs, ins = tiles[name, shape]
            assert st.tile_inputs(*shape) == ins, (name, shape)
            if name in TILE_OUTPUTS:
                assert TILE_OUTPUTS[name](*shape) == outs, (name, shape)
            if name in ("ddc", "ddc_bank", "pfb", "resamp", "resamp_bank"):
                assert ins * (shape[0] if two else 1) == outs * shape[-1], (name, shape)      # R (M / L) inputs per output
        for P in dims:
            shape = (P, 1) if two else (P,)
            for nt in range(1, 1025):
                want = hists[name, P, nt]
                assert sw._history(name, shape, nt) == want, (name, P, nt)
                if getattr(st, "history", None) is not None:
                    assert st.history(nt, *shape) == want, (name, P, nt)
