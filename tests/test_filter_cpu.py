"""ba_filter_track (host only, through ctypes) against the restatement of the rule (filter_checks.py) on the designed tracks: the
statuses are the fp64 restatement's, err_px and theta agree with it within 10 x its own distance from the long-double restatement plus
a few ulp; the parameter refusals; the defaults."""
import numpy as np
import pytest

import bundleadjustment_benchmarks_amd as ba
import filter_checks as FC

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("require_front", [True, False], ids=["front", "nofront"])
def test_host_rule_on_designed_cases(require_front):
    par = dict(FC.DEFAULTS, require_front=require_front)
    for c in FC.designed_cases(require_front):
        got = ba.filter_track(c["cams"], c["meas"], c["X"], active=c["active"], **par)
        r64, rld = FC.run_case(np.float64, c, **par), FC.run_case(FC.LD, c, **par)
        assert np.array_equal(got["obs_status"], r64["obs_status"]) and np.array_equal(got["obs_status"], c["expect_obs"]), (c["name"], got)
        assert got["pt_status"] == r64["pt_status"][0] == c["expect_pt"], (c["name"], got)
        on = c["active"]
        assert np.isnan(got["err_px"][~on]).all()
        fin = on & np.isfinite(rld["err"].astype(np.float64))
        assert not np.isfinite(got["err_px"][on & ~fin]).any()
        b = FC.err_bound(r64["err"][fin], rld["err"][fin], np.abs(c["meas"]).max(-1)[fin])
        d = np.abs(got["err_px"][fin] - rld["err"][fin].astype(np.float64))
        assert (d <= b).all(), (c["name"], d, b)
        # theta: the chord of two unit vectors, each rounded to a few eps: a few ulp of 1 rad on top of the restatement's own distance
        a64, ald = float(r64["angle_deg"][0]), float(rld["angle_deg"][0])
        ab = 10 * max(abs(a64 - ald), EPS * abs(ald)) + 8 * EPS * np.rad2deg(1.0)
        print("FILTER host %s err %.3e angle %.3e %.3e" % (c["name"], d.max() if len(d) else 0.0, abs(got["angle_deg"] - ald), ab))
        assert abs(got["angle_deg"] - ald) <= ab, (c["name"], got["angle_deg"], ald, ab)


def test_all_active_is_null():
    c = {q["name"]: q for q in FC.designed_cases()}["reproj"]
    a = ba.filter_track(c["cams"], c["meas"], c["X"])
    b = ba.filter_track(c["cams"], c["meas"], c["X"], active=np.ones(5, bool))
    assert np.array_equal(a["obs_status"], b["obs_status"]) and np.array_equal(a["err_px"], b["err_px"]) and a["angle_deg"] == b["angle_deg"]


def test_parameters_switch_the_steps_off():
    c = {q["name"]: q for q in FC.designed_cases()}
    assert ba.filter_track(c["reproj"]["cams"], c["reproj"]["meas"], c["reproj"]["X"], max_reproj_px=0.0)["obs_status"].tolist() == [0] * 5
    g = ba.filter_track(c["angle_half"]["cams"], c["angle_half"]["meas"], c["angle_half"]["X"], min_angle_deg=0.0)
    assert g["pt_status"] == ba.FPT_KEPT and g["angle_deg"] == 0.0 and g["obs_status"].tolist() == [0, 0]
    g = ba.filter_track(c["t1"]["cams"], c["t1"]["meas"], c["t1"]["X"], min_track=1, min_angle_deg=0.0)
    assert g["pt_status"] == ba.FPT_KEPT
    g = ba.filter_track(c["t0"]["cams"], c["t0"]["meas"], c["t0"]["X"], min_track=0, min_angle_deg=0.0)
    assert g["pt_status"] == ba.FPT_KEPT and len(g["obs_status"]) == 0


def test_refusals():
    c = {q["name"]: q for q in FC.designed_cases()}["t2"]
    bad = [dict(max_reproj_px=-1.0), dict(max_reproj_px=np.inf), dict(max_reproj_px=np.nan), dict(min_angle_deg=-0.1), dict(min_angle_deg=180.0),
           dict(min_angle_deg=np.nan), dict(min_angle_deg=np.inf), dict(min_track=-1)]
    for kw in bad:
        with pytest.raises(ba.BAError) as e:
            ba.filter_track(c["cams"], c["meas"], c["X"], **kw)
        assert e.value.code == ba.ERR_ARG, kw
    for kw in (dict(max_reproj_px=0.0), dict(min_angle_deg=0.0), dict(min_angle_deg=179.9), dict(min_track=0)):
        ba.filter_track(c["cams"], c["meas"], c["X"], **kw)
    L = ba.lib()
    X = np.zeros(3)
    assert L.ba_filter_track(-1, None, None, None, X.ctypes.data, None, None, None, None, None) == ba.ERR_ARG
    assert L.ba_filter_track(2, None, None, None, X.ctypes.data, None, None, None, None, None) == ba.ERR_ARG
    assert L.ba_filter_track(0, None, None, None, None, None, None, None, None, None) == ba.ERR_ARG
    assert L.ba_filter_track(0, None, None, None, X.ctypes.data, None, None, None, None, None) == 0  # (every output may be NULL)


def test_defaults_and_constants():
    p = ba.FilterParams.default()
    assert (p.max_reproj_px, p.min_angle_deg, p.min_track, p.require_front) == (4.0, 1.5, 2, 1)
    assert (ba.OBS_KEPT, ba.OBS_WAS_OFF, ba.OBS_BEHIND, ba.OBS_NONFINITE, ba.OBS_REPROJ, ba.OBS_POINT) == tuple(range(6))
    assert (ba.FPT_KEPT, ba.FPT_SHORT, ba.FPT_LOW_ANGLE) == (0, 1, 2)
    assert (FC.KEPT, FC.WAS_OFF, FC.BEHIND, FC.NONFINITE, FC.REPROJ, FC.POINT) == tuple(range(6))
    assert len(ba.OBS_NAMES) == 6 and len(ba.FPT_NAMES) == 3
