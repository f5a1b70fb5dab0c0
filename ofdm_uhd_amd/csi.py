"""Per-carrier channel report from the receiver's channel state, and a carrier map chosen from it.

The receive side of the reference's sense -> map -> transmit loop (sensing_and_tramsmitting*.py): the engine sums, per
occupied carrier, the preamble power, the decision error and reference energies and |1/eq|^2 over a call's packets
(Engine.rx_csi_summary, or ofdm_demod.carrier_report over a stream); carrier_report turns the sums into dB figures, and
suggest_carrier_map into a hex carrier map that ofdm_set_carrier_map / make_cfg(carriers=...) accept.  Definitions:
include/ofdm_hip.h (per-subcarrier channel state).
"""
import numpy as np

from . import config


def _cfg_dims(cfg):
    N, occ = int(cfg.fft_length), int(cfg.occupied_tones)
    cur = cfg.carrier_map
    cur = (cur.decode("ascii") if isinstance(cur, bytes) else cur) or "FE7F"
    return N, occ, cur


def _nearest_mean(values, src, dst):
    """At each index of dst: the mean of values at the nearest index of src on each side (one side at the band edge)."""
    src = np.asarray(src)
    out = np.empty(len(dst), np.float64)
    for k, i in enumerate(dst):
        lo = src[src < i]
        hi = src[src > i]
        v = []
        if len(lo):
            v.append(values[lo[-1]])
        if len(hi):
            v.append(values[hi[0]])
        out[k] = np.mean(v) if v else np.nan
    return out


def carrier_report(summary, cfg):
    """Per occupied carrier, from the float64 sums of rx_csi_summary / ofdm_demod.carrier_report's aggregate:
      P = pre_power / npkt; noise Nh = P at a null bin, at a pilot bin the mean of P at the nearest null bin on each side
      (one at the band edge); signal Sh = max(P - Nh, 0) at a pilot bin, at a null bin the mean of Sh at the neighbouring
      pilot bins;
      snr_preamble_db = 10 log10(max(Sh / Nh, 1e-6)) -- every occupied carrier, used by the current map or not;
      snr_decision_db = 10 log10(ref / max(err, 1e-30)) -- NaN outside the sink's current map;
      gain_db = 10 log10(mean |1/eq|^2).
    Returns a dict of float64 arrays [occupied_tones] (all NaN when npkt == 0)."""
    N, occ, cur = _cfg_dims(cfg)
    npkt = int(summary["npkt"])
    nan = np.full(occ, np.nan)
    if npkt == 0:
        return {"snr_preamble_db": nan.copy(), "snr_decision_db": nan.copy(), "gain_db": nan.copy()}
    ks = np.asarray(config.make_ksfreq(N, occ))
    pil, nul = np.flatnonzero(ks != 0), np.flatnonzero(ks == 0)
    P = np.asarray(summary["pre_power"], np.float64) / npkt
    Nh = np.empty(occ)
    Nh[nul] = P[nul]
    Nh[pil] = _nearest_mean(P, nul, pil)
    Sh = np.empty(occ)
    Sh[pil] = np.maximum(P[pil] - Nh[pil], 0.0)
    Sh[nul] = _nearest_mean(Sh, pil, nul)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr_pre = 10.0 * np.log10(np.maximum(Sh / Nh, 1e-6))
        err = np.asarray(summary["err"], np.float64)
        ref = np.asarray(summary["ref"], np.float64)
        snr_dd = 10.0 * np.log10(ref / np.maximum(err, 1e-30))
        ninv = np.asarray(summary["ninv"], np.float64)
        gain = 10.0 * np.log10(np.asarray(summary["inv_gain"], np.float64) / ninv)
    used = np.zeros(occ, bool)
    used[config.carrier_map(occ, occ, cur, sink=True)] = True
    snr_dd[~used] = np.nan
    gain[ninv == 0] = np.nan
    return {"snr_preamble_db": snr_pre, "snr_decision_db": snr_dd, "gain_db": gain}


def suggest_carrier_map(report, cfg, min_snr_db, respect_current=True):
    """Hex carrier map (config.carrier_map_hex) of the carriers whose preamble SNR, and decision SNR where they have one,
    reach min_snr_db.  respect_current: never enable a carrier the current map leaves off (e.g. the two DC carriers
    "FE7F" excludes).  ValueError if the set is empty, or if the map's growth rule would force on a carrier it
    excludes."""
    N, occ, cur = _cfg_dims(cfg)
    pre = np.asarray(report["snr_preamble_db"], np.float64)
    dd = np.asarray(report["snr_decision_db"], np.float64)
    on = (pre >= min_snr_db) & (np.isnan(dd) | (dd >= min_snr_db))
    if respect_current:
        cur_on = np.zeros(occ, bool)
        cur_on[config.carrier_map(occ, occ, cur, sink=True)] = True
        on &= cur_on
    return config.carrier_map_hex(occ, N, np.flatnonzero(on).tolist())
