"""Shared by test_resamp_bank_host.py and test_gpu_resamp_bank.py: the geometry of k_resamp_bank the tests pick their
sizes around, and the grids of the bit-identity and segmentation tests."""
import ddc_bank_cases
import resamp_cases

MAX_LINKS = 8
# eight centre frequencies (the fixed ones of the single stage's tests, 0.0 and 0.5 among them, three random ones and one
# duplicate), the K-link lists the grid picks from them, and the taps: the DDC bank's
frequencies, pick, taps_for = ddc_bank_cases.frequencies, ddc_bank_cases.pick, ddc_bank_cases.taps_for


def tile_inputs(L, M, K=1):
    """Inputs one workgroup of k_resamp_bank consumes: k_resamp's tile at every K (resamp_bank.h takes resamp_geom as
    it is; the links are taken in groups over one staged tile).  A wrong value here only moves the test sizes, it
    cannot make a wrong output pass."""
    return resamp_cases.tile_inputs(L, M)


def chains(L, M):
    """NG of the definition (include/ofdm_hip.h): 4 where L * KC < 4, 1 otherwise."""
    m = max(L, M)
    kc = 16 if m <= 1 else 8 if m <= 2 else 4 if m <= 4 else 2 if m <= 8 else 1
    return 4 if L * kc < 4 else 1


# (L, M) -> tap counts: at most three of {1, L - 1, 31, 155, 1024} per ratio, 1024 always at (64, 64), (1, 64) and
# (64, 1), the LDS extremes.  Both NG values ((1, 64) and (3, 25) have NG = 4), L > M, M > L, and phases without a tap
# (fewer taps than L)
TAP_GRID = {(1, 1): (1, 31, 1024), (2, 5): (1, 31, 155), (5, 2): (4, 155, 1024), (7, 1): (6, 31, 1),
            (8, 25): (7, 155, 1024), (3, 25): (2, 31, 1024), (1, 64): (1, 155, 1024), (64, 1): (63, 31, 1024),
            (64, 63): (63, 155, 1024), (63, 64): (62, 31, 1024), (64, 64): (1, 155, 1024)}
LINK_COUNTS = (1, 3, 8)

# (L, M, ntaps, K) of the segmentation test
SEG_SHAPES = [(2, 5, 39, 2), (4, 3, 23, 4), (8, 25, 481, 3), (64, 63, 1024, 8), (1, 64, 63, 5), (64, 1, 1024, 8),
              (3, 2, 2, 7), (5, 7, 1, 6)]


def stream_length(L, M):
    """min(2 tile + tile / 3 + 5, 60000) inputs, moved up to the next length that is a multiple of neither M nor the
    tile."""
    tile = tile_inputs(L, M)
    n = min(2 * tile + tile // 3 + 5, 60000)
    while (M > 1 and n % M == 0) or n % tile == 0:
        n += 1
    return n


def far_start(M):
    """A stream origin near 10^6 that is no multiple of M."""
    return 1000003 if 1000003 % M else 1000004
