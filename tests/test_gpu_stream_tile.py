"""Tile staging of the wideband stages (every kernel has the block in its own text: DESIGN.md, "The eight
wideband stages share one host-side skeleton ..."): a
call's first tile takes the carried history, its last tile zeros behind the call's end, and a tile in between moves
16-byte pairs on the 16-byte grid of the CALLER's buffer, so the pair a lane loads begins on an even or an odd sample of
the tile depending on where the buffer lies.  Every stage that stages in pairs runs one call of three tiles and a few
samples twice through device pointers -- its input on a 16-byte boundary, and 8 bytes behind one -- and must give the
bits of the host-mode call (whose device copy of the input is the library's own) both times."""
import numpy as np
import pytest

import ddc_cases
import pfb_cases
import pfb_synth_cases
import resamp_cases
import tx_resamp_cases
from helpers import make_cfg
from ofdm_uhd_amd import ddc, engine, pfb, resample, tx_resample

pytestmark = pytest.mark.gpu

EXTRA = 37  # samples past the third tile


def _taps(rng, n):
    return (rng.standard_normal(n) / np.sqrt(n)).astype(np.float32)


def _stages():
    """name -> (configuration, input samples of one tile, input rows, output rows): the smallest tile of each stage."""
    rng = np.random.default_rng(5)
    return {
        "ddc": (ddc.ddc_cfg(17, 0.21, taps=_taps(rng, 40)), ddc_cases.tile_outputs(17) * 17, 0, 0),
        "ddc_bank": (ddc.bank_cfg(17, [-0.3, 0.12, 0.4], taps=_taps(rng, 40)), ddc_cases.tile_outputs(17) * 17, 0, 3),
        "pfb": (pfb.pfb_cfg(4, channels=[1, 3], taps=_taps(rng, 23)), pfb_cases.tile_outputs(4) * 4, 0, 2),
        "resamp": (resample.resamp_cfg(3, 10, -0.17, taps=_taps(rng, 31)), resamp_cases.tile_inputs(3, 10), 0, 0),
        "tx_resamp": (tx_resample.tx_resamp_cfg(9, 10, -0.2, taps=_taps(rng, 50)), tx_resamp_cases.tile_inputs(9, 10), 0, 0),
        "pfb_synth": (pfb.synth_cfg(64, [1, 40], taps=_taps(rng, 200)), pfb_synth_cases.tile_inputs(64), 2, 0),
    }


CASES = [(s, f) for s in ("ddc", "ddc_bank", "pfb", "resamp") for f in ("fc32", "sc16")] + [("tx_resamp", "fc32"), ("pfb_synth", "fc32")]


@pytest.mark.parametrize("stage,fmt", CASES)
def test_both_parities_of_the_input_pointer(stage, fmt):
    import torch
    dev = torch.device("cuda", 0)
    cfg, tile, rows_in, rows_out = _stages()[stage]
    n = 3 * tile + EXTRA
    rng = np.random.default_rng(11)
    if fmt == "sc16":
        raw = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    else:
        shape = (rows_in, n) if rows_in else (n,)
        raw = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    per = 4 if fmt == "sc16" else 8  # bytes per input sample

    host = engine.Engine(cfg=make_cfg())
    devE = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        for e in (host, devE):
            if stage not in ("tx_resamp", "pfb_synth"):
                e.set_rx_iq_format(fmt)
            getattr(e, "set_" + stage)(cfg)
        want = getattr(host, stage)(raw)
        assert want.size > 0
        no = want.shape[-1] if rows_out else len(want)
        for shift in (0, 8):
            # the samples `shift` bytes behind a 16-byte boundary (torch's allocations begin on one); a row of a bank's
            # input is a whole number of 16-byte words long, so every row has the parity of the first
            width = (n * per + shift + 15) // 16 * 16
            buf = torch.zeros((max(rows_in, 1), width), dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0
            src = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(max(rows_in, 1), n * per)).to(dev)
            buf[:, shift:shift + n * per] = src
            y = torch.zeros((max(rows_out, 1), no), dtype=torch.complex64, device=dev)
            getattr(devE, stage + "_reset")(0)
            x_ptr = buf.data_ptr() + shift
            if stage in ("ddc", "resamp", "tx_resamp"):
                got = getattr(devE, stage + "_device")(x_ptr, n, y.data_ptr(), no)
            elif stage == "pfb_synth":
                got = devE.pfb_synth_device(x_ptr, width // 8, n, y.data_ptr(), no)
            else:
                got = getattr(devE, stage + "_device")(x_ptr, n, y.data_ptr(), no, no)
            torch.cuda.synchronize()
            out = y.cpu().numpy()
            assert got == no, (stage, fmt, shift)
            assert np.array_equal(out if rows_out else out[0], want), (stage, fmt, shift)
            # (handed back zeroed: a later test's torch.empty() must not inherit these bytes)
            for t in (buf, src, y):
                t.zero_()
            torch.cuda.synchronize()
            del buf, src, y
        torch.cuda.empty_cache()
    finally:
        host.close()
        devE.close()
