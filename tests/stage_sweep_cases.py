"""Shared by test_stage_sweep_cases_host.py and test_gpu_stage_sweep.py: a seeded, stratified sweep over the whole
configuration space the ten wideband stream stages accept.  cases(stage) is deterministic from SEEDS[stage]; a case is
(shape, ntaps, selection, first index, stream length, one chunking) and, for a transmit stage, the input amplitude that
keeps the float64 model below half of the 16-bit full scale.  Nothing here needs a GPU.

The classes.  classes_of() restates, per stage, every template instantiation and every branch on (L, M, R, ntaps, K)
of the staging, filter and store loops; CLASSES lists the labels, and every label has a case (the host test checks it).

  ddc (ddc.h, engine_ddc.inc)
    geom:opt4_tj256 | opt4_tj64 | opt1_tj64    ddc_geom: R <= 4 | R <= 16 | R > 16 (boundaries R = 4|5, 16|17)
    taps:one_row | rows                        Q = (ntaps - 1) / R is 0 | more (the qq loop runs once | more)
    taps:full_rows | remainder_row             np = min(R, ntaps - k0): ntaps a multiple of R | not
    chains:idle | all_work                     NG = 4 only: Q + 1 < NG, chains without a row | every chain has one
    lds:combine_larger | samples_larger        NG = 4 only: which of the two overlaid regions sets ddc_lds_bytes
  ddc_bank (ddc_bank.h): ddc's geom, taps and chains, and
    links:lg4_of4 lg2_of4 lg1_of4              the passes of k_ddc_bank<.., OPT = 4>: K in groups of 4, then 2, then 1
    links:lg8_of8 lg4_of8 lg2_of8 lg1_of8      ... and of OPT = 1: groups of 8, 4, 2, 1
  resamp (resamp.h)
    geom:kc16_ng1 kc8_ng1 kc4_ng1 kc2_ng1 kc2_ng4 kc1_ng1 kc1_ng4     resamp_geom: max(L, M) <= 1, 2, 4, 8, more;
                                               NG = 4 where L KC < 4 (boundaries max = 1|2, 2|3, 4|5, 8|9; L = 1|2 at
                                               M in 5..8; L = 3|4 at M > 8)
    ratio:up | down | one                      L > M | L < M | L = M (off = r M / L and the row walk differ)
    rows:M1 | many                             M = 1: every tap steps one column back | the row index wraps
    hist:none | one_period | periods           Q = 0 | QM = ceil(Q / M) = 1 | more
    taps:phase_without_tap                     ntaps < L: nq = 0 for some phase
    taps:full | ragged                         ntaps a multiple of L | phases with different tap counts
    chains:idle | all_work                     NG = 4 only: fewer than 4 taps per phase | not
  resamp_bank (resamp_bank.h): resamp's, and
    sums:nb1 nb2 nb4 nb8                       resamp_bank_sum_links: links the sum buffer holds
    sums:half | whole                          ... inside half the LDS | only inside the whole 160 KB
    links:lg8 lg4 lg2 lg1                      the passes of k_resamp_bank: min(K - l0, NB) in groups of 8, 4, 2, 1
  pfb (pfb.h)
    M:2 .. M:64                                k_pfb<XT, M>; M >= 32: the transform in two steps, T < 256 (p0 = tid / T)
    hist:none | some                           Q = 0: the full-row loop does not run
    taps:full | ragged                         the last row of taps holds every branch | some
    taps:branch_without_tap                    ntaps < M
    sel:one | some | all | repeat              pfb_store walks first[] / next[]: one row, several, every channel, a
                                               channel kept twice
  pfb_synth (pfb_synth.h)
    M:2 .. M:64                                k_pfb_synth<OUT, ADD, M>; M >= 32: 64-lane staging groups, odd pitch, two
                                               transform steps; M < 32: 256 lanes, pitch = 32 / M (mod 32)
    hist, taps                                 as pfb (the last row under `Q M + p < ntaps`)
    sel:one | some | all                       rows of channels not selected are zeroed | none is
  duc (duc.h)
    geom:opt8 | opt4                           duc_geom: L <= 2 | more (boundary L = 2|3)
    hist:none | some, taps:full | ragged, taps:phase_without_tap      left[i] = taps of the output's phase
  duc_bank (duc_bank.h): duc's, and
    phase:shared | per_output                  L divides 256: one tap read serves a thread's outputs | not
    rows:none_full | full                      Qf = ntaps / L is 0 | more (the loop without a per-output test)
    tail:none | rem                            ntaps - Qf L: the row under `ph < rem`
    links:one | many
  tx_resamp (tx_resamp.h)
    geom:kc1 kc2 kc4 kc8 kc16                  tx_resamp_geom: resamp_geom's KC, doubled while L KC < 4 and the tile
    geom:widened | as_resamp                   stays within 4096 inputs
    ratio, rows, hist, taps                    as resamp
  tx_resamp_bank (tx_resamp_bank.h): tx_resamp's, and
    group:1 2 3 4                              tx_resamp_bank_group<NG>: outputs of a period that share their reads
    group:skip                                 a slot without an output (ng <= 0)
    slots:one | many                           more than 4 outputs per newest input (L > 4 M)
    links:one | many

Every case of a receive stage in fc32 and of tx_resamp and pfb_synth has an interior tile, which is where the 16-byte
load sits; the GPU test runs those through device pointers at both parities of the input pointer."""
import collections
import functools

import numpy as np

import ddc_bank_cases
import duc_bank_cases
import stage_harness as sh
from ofdm_uhd_amd import ddc, resample

STAGE_NAMES = ("ddc", "ddc_bank", "resamp", "resamp_bank", "pfb", "pfb_synth", "duc", "duc_bank", "tx_resamp",
               "tx_resamp_bank")
SEED = 20261
SEEDS = {name: SEED + 97 * i for i, name in enumerate(STAGE_NAMES)}
RANDOM_CASES = 16
HALF_SCALE = 0.5                   # the float64 model's peak stays below this (full scale is 1.0)
LDS_MAX = 160 * 1024               # RESAMP_BANK_LDS_MAX (resamp_bank.h)

Case = collections.namedtuple("Case", "stage idx why shape ntaps sel first n chunks seed amp")

_PFB_M = (2, 4, 8, 16, 32, 64)
_EDGE = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64)


# ---- the classes, restated from the headers ---------------------------------------------------------------------------

def _resamp_kc(L, M):
    m = max(L, M)
    return 16 if m <= 1 else 8 if m <= 2 else 4 if m <= 4 else 2 if m <= 8 else 1


def _tx_kc(L, M):
    kc = _resamp_kc(L, M)
    while L * kc < 4 and 2 * kc * 64 * M <= 4096:
        kc *= 2
    return kc


def _ddc_geom(R):
    return ("opt4_tj256", 4, 256, 1) if R <= 4 else ("opt4_tj64", 4, 64, 4) if R <= 16 else ("opt1_tj64", 1, 64, 4)


def _ddc_classes(R, ntaps, K=None):
    name, opt, tj, NG = _ddc_geom(R)
    T, Q = opt * tj, (ntaps - 1) // R
    c = {"geom:" + name, "taps:one_row" if Q == 0 else "taps:rows",
         "taps:full_rows" if ntaps % R == 0 else "taps:remainder_row"}
    if NG > 1:
        c.add("chains:idle" if Q + 1 < NG else "chains:all_work")
        if K is None:
            c.add("lds:combine_larger" if NG * T * 16 > R * ((T + Q) | 1) * 8 else "lds:samples_larger")
    if K is not None:
        top, left = (4 if opt == 4 else 8), K
        for lg in (8, 4, 2, 1):
            if lg > top:
                continue
            if lg == top and left >= lg:
                c.add("links:lg%d_of%d" % (lg, top))
                left %= lg
            elif left >= lg:
                c.add("links:lg%d_of%d" % (lg, top))
                left -= lg
    return c


def _taps_classes(L, ntaps):
    c = {"taps:full" if ntaps % L == 0 else "taps:ragged"}
    if ntaps < L:
        c.add("taps:phase_without_tap")
    return c


def _ratio_classes(L, M, ntaps):
    Q = (ntaps - 1) // L
    QM = -(-Q // M)
    c = {"ratio:up" if L > M else "ratio:down" if L < M else "ratio:one", "rows:M1" if M == 1 else "rows:many",
         "hist:none" if Q == 0 else "hist:one_period" if QM == 1 else "hist:periods"}
    return c | _taps_classes(L, ntaps)


def _resamp_classes(L, M, ntaps):
    kc = _resamp_kc(L, M)
    ng = 4 if L * kc < 4 else 1
    c = {"geom:kc%d_ng%d" % (kc, ng)} | _ratio_classes(L, M, ntaps)
    if ng > 1:
        c.add("chains:idle" if -(-ntaps // L) < ng else "chains:all_work")
    return c


def resamp_bank_sum_links(L, M, ntaps, K):
    """(NB, budget) of resamp_bank_sum_links (resamp_bank.h), restated."""
    kc = _resamp_kc(L, M)
    ng, TJ = (4 if L * kc < 4 else 1), 64 * kc
    QM = -(-((ntaps - 1) // L) // M)
    words = ntaps * ((K + 1) & ~1) + ((M * ((TJ + QM) | 1) + 1) & ~1)
    per_link = ng * TJ * L * 2 if ng > 1 else L * (TJ | 1)
    for budget in (LDS_MAX // 2, LDS_MAX):
        for nb in (8, 4, 2, 1):
            if nb <= K and (words + nb * per_link) * 8 <= budget:
                return nb, budget
    return 1, LDS_MAX


def _resamp_bank_classes(L, M, ntaps, K):
    c = _resamp_classes(L, M, ntaps)
    nb, budget = resamp_bank_sum_links(L, M, ntaps, K)
    c |= {"sums:nb%d" % nb, "sums:half" if budget < LDS_MAX else "sums:whole"}
    l0 = 0
    while l0 < K:
        cap = min(K - l0, nb)
        lg = 8 if cap >= 8 else 4 if cap >= 4 else 2 if cap >= 2 else 1
        c.add("links:lg%d" % lg)
        l0 += lg
    return c


def _pfb_classes(M, ntaps, chans, synth):
    Q = (ntaps - 1) // M
    c = {"M:%d" % M, "hist:none" if Q == 0 else "hist:some", "taps:full" if ntaps % M == 0 else "taps:ragged"}
    if ntaps < M:
        c.add("taps:branch_without_tap")
    if len(set(chans)) < len(chans):
        c.add("sel:repeat")
    c.add("sel:one" if len(chans) == 1 else "sel:all" if len(set(chans)) == M else "sel:some")
    assert not (synth and "sel:repeat" in c)
    return c


def _duc_classes(L, ntaps):
    return ({"geom:opt8" if L <= 2 else "geom:opt4", "hist:none" if (ntaps - 1) // L == 0 else "hist:some"}
            | _taps_classes(L, ntaps))


def _duc_bank_classes(L, ntaps, K):
    Qf = ntaps // L
    return _duc_classes(L, ntaps) | {"phase:shared" if 256 % L == 0 else "phase:per_output",
                                     "rows:none_full" if Qf == 0 else "rows:full",
                                     "tail:rem" if ntaps - Qf * L else "tail:none", "links:one" if K == 1 else "links:many"}


def _tx_resamp_classes(L, M, ntaps):
    kc = _tx_kc(L, M)
    return ({"geom:kc%d" % kc, "geom:widened" if kc > _resamp_kc(L, M) else "geom:as_resamp"}
            | _ratio_classes(L, M, ntaps))


def _tx_resamp_bank_classes(L, M, ntaps, K):
    c = _tx_resamp_classes(L, M, ntaps)
    slots = (-(-L // M) + 3) // 4
    c |= {"slots:many" if slots > 1 else "slots:one", "links:one" if K == 1 else "links:many"}
    for off in range(M):
        for slot in range(slots):
            rb = (off * L + M - 1) // M + slot * 4
            re = min(((off + 1) * L + M - 1) // M, L)
            ng = min(re - rb, 4)
            c.add("group:skip" if ng <= 0 else "group:%d" % ng)
    return c


def classes_of(stage, shape, ntaps, sel):
    """The labels of one configuration (see the module docstring)."""
    if stage == "ddc":
        return _ddc_classes(shape[0], ntaps)
    if stage == "ddc_bank":
        return _ddc_classes(shape[0], ntaps, len(sel))
    if stage == "resamp":
        return _resamp_classes(*shape, ntaps)
    if stage == "resamp_bank":
        return _resamp_bank_classes(*shape, ntaps, len(sel))
    if stage in ("pfb", "pfb_synth"):
        return _pfb_classes(shape[0], ntaps, sel, stage == "pfb_synth")
    if stage == "duc":
        return _duc_classes(shape[0], ntaps)
    if stage == "duc_bank":
        return _duc_bank_classes(shape[0], ntaps, len(sel))
    if stage == "tx_resamp":
        return _tx_resamp_classes(*shape, ntaps)
    return _tx_resamp_bank_classes(*shape, ntaps, len(sel))


_DDC = ("geom:opt4_tj256", "geom:opt4_tj64", "geom:opt1_tj64", "taps:one_row", "taps:rows", "taps:full_rows",
        "taps:remainder_row", "chains:idle", "chains:all_work")
_RATIO = ("ratio:up", "ratio:down", "ratio:one", "rows:M1", "rows:many", "hist:none", "hist:one_period", "hist:periods",
          "taps:phase_without_tap", "taps:full", "taps:ragged")
_RESAMP = ("geom:kc16_ng1", "geom:kc8_ng1", "geom:kc4_ng1", "geom:kc2_ng1", "geom:kc2_ng4", "geom:kc1_ng1",
           "geom:kc1_ng4", "chains:idle", "chains:all_work") + _RATIO
_PFB = tuple("M:%d" % m for m in _PFB_M) + ("hist:none", "hist:some", "taps:full", "taps:ragged",
                                             "taps:branch_without_tap", "sel:one", "sel:some", "sel:all")
_DUC = ("geom:opt8", "geom:opt4", "hist:none", "hist:some", "taps:full", "taps:ragged", "taps:phase_without_tap")
_TXR = ("geom:kc1", "geom:kc2", "geom:kc4", "geom:kc8", "geom:kc16", "geom:widened", "geom:as_resamp") + _RATIO
CLASSES = {
    "ddc": _DDC + ("lds:combine_larger", "lds:samples_larger"),
    "ddc_bank": _DDC + ("links:lg4_of4", "links:lg2_of4", "links:lg1_of4", "links:lg8_of8", "links:lg4_of8",
                        "links:lg2_of8", "links:lg1_of8"),
    "resamp": _RESAMP,
    "resamp_bank": _RESAMP + ("sums:nb1", "sums:nb2", "sums:nb4", "sums:nb8", "sums:half", "sums:whole", "links:lg8",
                              "links:lg4", "links:lg2", "links:lg1"),
    "pfb": _PFB + ("sel:repeat",),
    "pfb_synth": _PFB,
    "duc": _DUC,
    "duc_bank": _DUC + ("phase:shared", "phase:per_output", "rows:none_full", "rows:full", "tail:none", "tail:rem",
                        "links:one", "links:many"),
    "tx_resamp": _TXR,
    "tx_resamp_bank": _TXR + ("group:1", "group:2", "group:3", "group:4", "group:skip", "slots:one", "slots:many",
                              "links:one", "links:many"),
}

# one shape on each side of every boundary between geometry classes
_LM_EDGES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3), (4, 4), (5, 4), (4, 5), (8, 8), (9, 8), (8, 9),       # max(L, M)
             (1, 4), (1, 5), (1, 8), (2, 8), (1, 9), (3, 9), (4, 9), (3, 64), (4, 64),                              # L KC < 4
             (1, 16), (1, 17), (1, 32), (1, 33), (2, 16), (2, 17), (3, 10), (3, 11),                               # the widened tile
             (64, 1), (64, 64), (63, 64), (64, 63), (17, 4), (16, 4)]                                              # ratio, slots
BOUNDARY_SHAPES = {
    "ddc": [(1,), (4,), (5,), (16,), (17,), (64,)],
    "ddc_bank": [(1,), (4,), (5,), (16,), (17,), (64,)],
    "resamp": _LM_EDGES, "resamp_bank": _LM_EDGES, "tx_resamp": _LM_EDGES, "tx_resamp_bank": _LM_EDGES,
    "pfb": [(m,) for m in _PFB_M], "pfb_synth": [(m,) for m in _PFB_M],
    "duc": [(1,), (2,), (3,), (64,)],
    "duc_bank": [(1,), (2,), (3,), (32,), (33,), (63,), (64,)],                # ... and L divides 256 | does not
}


# ---- drawing configurations -------------------------------------------------------------------------------------------

def _bank(stage):
    return sh.STAGES[stage].rows is not None


def _channels(stage):
    return stage in ("pfb", "pfb_synth")


def _poly(stage, shape):
    """P: what the stage divides its taps by (R, L or M)."""
    return shape[0]


def _period(stage, shape):
    return shape[-1] if len(shape) == 2 else shape[0]


def _draw_dim(rng):
    return int(rng.choice(_EDGE)) if rng.random() < 0.5 else int(rng.integers(1, 65))


def _draw_shape(rng, stage):
    if _channels(stage):
        return (int(rng.choice(_PFB_M)),)
    return tuple(_draw_dim(rng) for _ in range(2 if stage in ("resamp", "resamp_bank", "tx_resamp", "tx_resamp_bank") else 1))


def _draw_ntaps(rng, P):
    if rng.random() < 0.5:
        k = int(rng.integers(1, max(1024 // P, 1) + 1))
        return int(min(max(rng.choice([1, P - 1, P, P + 1, k * P - 1, k * P, k * P + 1, 3 * P, 3 * P + 1, 1023, 1024]), 1), 1024))
    return int(rng.integers(1, 1025))


def _draw_sel(rng, stage, shape, i, K=None):
    """A centre frequency, K of them, or a channel selection; ``i`` rotates the special values through the list."""
    if _channels(stage):
        M = shape[0]
        kind = int(rng.integers(0, 4))
        n = 1 if kind == 0 else M if kind == 1 else int(rng.integers(1, min(M, 8) + 1))
        chans = [int(c) for c in rng.permutation(M)[:n]]
        must = (0, M // 2, M - 1)[i % 3]
        if must not in chans:
            chans[int(rng.integers(0, n))] = must
        if stage == "pfb" and n >= 2 and n < M and i % 4 == 3:
            chans.append(chans[0])                          # a channel kept twice
        return tuple(chans)
    special = (0.0, 0.5, -0.5)[i % 11] if i % 11 < 3 else None      # (most frequencies are random: 0 and +-0.5 hide a sign)
    if not _bank(stage):
        return float(rng.uniform(-0.5, 0.5)) if special is None else special
    K = int(rng.integers(1, 9)) if K is None else K
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, K)]
    if special is not None:
        fcs[int(rng.integers(0, K))] = special
    elif K >= 2 and i % 5 == 3:
        fcs[K - 1] = fcs[0]                                 # one duplicated frequency
    return tuple(fcs)


def _history(stage, shape, ntaps):
    """Samples before a call's first that its outputs reach, in input samples (per row)."""
    if stage in ("ddc", "ddc_bank", "pfb"):
        return ntaps - 1
    return (ntaps - 1) // shape[0]


def _tile(stage, shape):
    return int(sh.STAGES[stage].tile_inputs(*shape))


def _length(stage, shape, ntaps):
    """The smallest stream with a first (edge) tile, an interior tile and a partial last one: 2.5 tiles and the
    history, moved up to a length that is a multiple of neither the period nor the tile."""
    tile, per = _tile(stage, shape), _period(stage, shape)
    n = 5 * tile // 2 + _history(stage, shape, ntaps) + 3
    while (per > 1 and n % per == 0) or (tile > 1 and n % tile == 0):
        n += 1
    return n


def _first(stage, shape, n, kind):
    st = sh.STAGES[stage]
    per = max(shape)
    if kind == "small" or (st.phase_free and kind != "zero"):
        return 7 * per + 1 if per > 1 else 8
    return {"zero": 0, "start": sh.START, "far": sh.FAR, "limit": st.index_limit(*shape) - n - 1}[kind]


_FIRSTS = ("zero", "small", "start", "far", "limit")


def _chunks(rng, stage, shape, ntaps, first, n):
    """0, 1, P - 1, P + 1, tile - 1, tile + 1 (each while it fits), then random sizes up to a tile; and one call that
    completes no output where the stage can have one."""
    st, P, tile = sh.STAGES[stage], _poly(stage, shape), _tile(stage, shape)
    out, left = [0], n
    for s in (1, P - 1, P + 1, tile - 1, tile + 1):
        s = min(s, left)
        if s >= 1:
            out.append(s)
            left -= s
    while left:
        s = min(int(rng.integers(1, tile + 2)), left)
        out.append(s)
        left -= s
    at = [sum(out[:k]) for k in range(len(out))]
    if not any(s and st.count(first + a, s, *shape) == 0 for a, s in zip(at, out)):
        # cut a long chunk where a single sample completes nothing (a decimating stage has such a sample in every period)
        k = int(np.argmax(out))
        for j in range(1, min(2 * max(shape) + 2, out[k] - 1)):
            if st.count(first + at[k] + j, 1, *shape) == 0:
                out[k:k + 1] = [j, 1, out[k] - j - 1]
                break
    assert sum(out) == n and min(out) >= 0
    return tuple(int(s) for s in out)


def taps_of(case):
    rng = np.random.default_rng(case.seed)
    if sh.STAGES[case.stage].side == "rx":
        return ddc_bank_cases.taps_for(rng, case.ntaps)
    return duc_bank_cases.taps_for(rng, case.ntaps)


def rx_input(case, fmt):
    """(samples in the receive format, the same as complex64)."""
    return sh.rx_stream(np.random.default_rng(case.seed + 1), case.n, fmt)


def tx_input(case):
    """The K rows of a transmit bank's input (one row, 1-D, for a single stage) at the case's amplitude."""
    x = _tx_unit_input(case.stage, case.seed, case.n, 1 if not _bank(case.stage) else len(case.sel))
    x = (x * np.float32(case.amp)).astype(np.complex64)         # a power of two: exact
    return x if _bank(case.stage) else x[0]


def tx_add(case, nout):
    """The band a transmit case is run onto once more."""
    return sh.rows(np.random.default_rng(case.seed + 2), 1, nout, amp=0.125)[0]


def _tx_unit_input(stage, seed, n, K):
    return sh.rows(np.random.default_rng(seed + 1), K, n, amp=1.0)


def tx_model(stage, shape, taps, sel, first, x):
    """(y64, s) of a transmit stage for the rows x."""
    st = sh.STAGES[stage]
    if stage == "pfb_synth":
        return st.cases.model(x, taps, *shape, sel)
    if _bank(stage):
        return st.cases.model(x, taps, *shape, list(sel), first)
    return st.cases.model(np.asarray(x).reshape(-1), taps, *shape, st.cases.phase_step(sel), first)


def _tx_amp(stage, shape, ntaps, sel, first, n, seed):
    """The largest power of two that keeps the float64 model's peak, per part, below HALF_SCALE."""
    case = Case(stage, 0, "", shape, ntaps, sel, first, n, (), seed, 1.0)
    y64, _ = tx_model(stage, shape, taps_of(case), sel, first, _tx_unit_input(stage, seed, n, len(sel) if _bank(stage) else 1))
    peak = float(max(np.max(np.abs(y64.real)), np.max(np.abs(y64.imag)), 1e-30)) if len(y64) else 1.0
    return float(2.0 ** np.floor(np.log2(HALF_SCALE * 0.999 / peak)))


def rx_table(case, link=None):
    """The normative table of a receive stage's link (what Engine.<stage>_taps returns)."""
    fc = case.sel if link is None else case.sel[link]
    if case.stage in ("ddc", "ddc_bank"):
        return ddc.bandpass_taps(taps_of(case), fc)
    return resample.bandpass_taps(taps_of(case), fc, case.shape[0])


def _make(rng, stage, i, why, shape, ntaps, sel, first_kind):
    n = _length(stage, shape, ntaps)
    first = _first(stage, shape, n, first_kind)
    seed = int(rng.integers(1, 1 << 30))
    chunks = _chunks(rng, stage, shape, ntaps, first, n)
    amp = _tx_amp(stage, shape, ntaps, sel, first, n, seed) if sh.STAGES[stage].side == "tx" else 1.0
    return Case(stage, i, why, shape, ntaps, sel, first, n, chunks, seed, amp)


def _ntaps_flips(stage, shape, sel):
    """{label: ntaps}: the smallest ntaps > 1 at which the label's membership changes at this shape (ragged | full
    change at every row and are left to the P-relative values)."""
    skip = ("taps:full", "taps:ragged", "taps:full_rows", "taps:remainder_row")
    flips, prev = {}, classes_of(stage, shape, 1, sel)
    for nt in range(2, 1025):
        cur = classes_of(stage, shape, nt, sel)
        for lab in (cur ^ prev):
            if lab not in skip:
                flips.setdefault(lab, nt)
        prev = cur
    return flips


@functools.lru_cache(maxsize=None)
def cases(stage):
    """The stage's cases: the boundary shapes crossed with the P-relative tap counts, both sides of every ntaps class
    boundary, one case for every class still without one, then RANDOM_CASES uniformly random configurations."""
    rng = np.random.default_rng(SEEDS[stage])
    out, bank_K = [], (1, 3, 8, 2, 5, 7, 4, 6)

    def add(why, shape, ntaps, sel=None, K=None):
        i = len(out)
        if sel is None:
            sel = _draw_sel(rng, stage, shape, i, K if K is not None else bank_K[i % 8] if _bank(stage) and not _channels(stage) else None)
        out.append(_make(rng, stage, i, why, shape, int(ntaps), sel, _FIRSTS[i % len(_FIRSTS)]))

    shapes = BOUNDARY_SHAPES[stage]
    kinds = ("1", "P-1", "P", "P+1", "kP-1", "kP", "kP+1", "1024", "random", "random")
    for i in range(max(len(shapes), len(kinds))):
        shape, kind = shapes[i % len(shapes)], kinds[i % len(kinds)]
        P = _poly(stage, shape)
        k = int(rng.integers(2, max(1024 // P, 2) + 1))
        nt = {"1": 1, "P-1": P - 1, "P": P, "P+1": P + 1, "kP-1": k * P - 1, "kP": k * P, "kP+1": k * P + 1, "1024": 1024,
              "random": int(rng.integers(1, 1025))}[kind]
        add("shape %s, ntaps %s" % (shape, kind), shape, min(max(nt, 1), 1024))
    # both sides of every ntaps class boundary, at the first boundary shape that has it
    seen = set()
    for shape in shapes:
        sel = _draw_sel(rng, stage, shape, len(out), 8 if _bank(stage) and not _channels(stage) else None)
        for lab, nt in sorted(_ntaps_flips(stage, shape, sel).items()):
            if lab not in seen:
                seen.add(lab)
                if (shape, nt) not in seen:             # (two labels may change at the same count)
                    seen.add((shape, nt))
                    add("below the ntaps boundary of %s" % lab, shape, nt - 1, sel)
                    add("above the ntaps boundary of %s" % lab, shape, nt, sel)
    # every class still without a case
    have = set().union(*(classes_of(stage, c.shape, c.ntaps, c.sel) for c in out))
    for lab in CLASSES[stage]:
        if lab in have:
            continue
        for _ in range(200000):
            shape = _draw_shape(rng, stage)
            nt = _draw_ntaps(rng, _poly(stage, shape))
            sel = _draw_sel(rng, stage, shape, int(rng.integers(0, 60)))
            if lab in classes_of(stage, shape, nt, sel):
                break
        else:
            raise AssertionError("no configuration of %s drawn in class %s" % (stage, lab))
        add("class %s" % lab, shape, nt, sel)
        have |= classes_of(stage, shape, nt, sel)
    for _ in range(RANDOM_CASES):
        shape = (int(rng.choice(_PFB_M)),) if _channels(stage) else tuple(int(rng.integers(1, 65)) for _ in BOUNDARY_SHAPES[stage][0])
        add("random", shape, int(rng.integers(1, 1025)))
    return tuple(out)


def cfg_of(case, out_format=None):
    """The case's configuration from the stage's cfg builder."""
    st = sh.STAGES[case.stage]
    sel = list(case.sel) if isinstance(case.sel, tuple) else case.sel
    kw = {} if out_format is None else {"out_format": out_format}
    return st.cfg(*case.shape, sel, taps=taps_of(case), **kw)
