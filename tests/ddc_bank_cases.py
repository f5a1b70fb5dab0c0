"""Shared by test_ddc_bank_host.py and test_gpu_ddc_bank.py: the geometry of k_ddc_bank the tests pick their sizes
around, and the grid of the bit-identity test."""
import numpy as np

import ddc_cases

MAX_LINKS = 8


def tile_outputs(R, K=1):
    """Outputs per link one workgroup of k_ddc_bank produces: k_ddc's tile at every K (ddc_bank.h takes ddc_geom as it
    is; the links are taken in groups over one staged tile).  A wrong value here only moves the test sizes, it cannot
    make a wrong output pass."""
    return ddc_cases.tile_outputs(R)


# decimation -> tap counts: at most three of {1, R - 1, 31, 155, 1024} per R, 1024 always at R = 2 and R = 64
TAP_GRID = {1: (1, 31, 1024), 2: (1, 155, 1024), 3: (2, 31, 155), 4: (3, 31, 1024), 5: (4, 155, 1), 8: (7, 155, 1024),
            17: (16, 31, 1), 64: (63, 155, 1024)}
LINK_COUNTS = (1, 3, 8)


def frequencies(rng, fixed):
    """Eight centre frequencies: the fixed ones of the DDC's tests, three random ones, and one duplicate."""
    f = list(fixed) + [float(v) for v in rng.uniform(-0.5, 0.5, MAX_LINKS - 1 - len(fixed))]
    return f + [f[2]]


def pick(freqs, K):
    """The K-link list the grid uses: K = 3 holds the duplicate pair, K = 1 a random frequency."""
    return {1: [freqs[5]], 3: [freqs[2], freqs[4], freqs[7]], 8: list(freqs)}[K]


def stream_length(R):
    tile = tile_outputs(R) * R
    n = min(2 * tile + tile // 3 + 5, 60000)
    while (R > 1 and n % R == 0) or n % tile == 0 or n % (ddc_cases.tile_outputs(R) * R) == 0:
        n += 1
    return n


def taps_for(rng, ntaps):
    return (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
