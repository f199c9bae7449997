"""The SBS output's host twin (msd_pos_host_sbs_enable, msd_pos_host_update_sbs, msd_pos_host_sbs_wire: the walk of
msd_trk_impl.h with its hand-over rows, the text from snprintf / gmtime_r / atan2) on the CPU: the twin == the second
reading of tests/indep_sbs.py == the lines written out by hand in tests/sbs_streams.py, one scenario per rule, and the
three agree on the aircraft table's mixed stream.  The GPU is held against the twin in test_gpu_sbs.py."""
import errno

import numpy as np
import pytest

import aircraft_streams as acs
import indep_sbs as isbs
import sbs_streams as ss


@pytest.fixture(scope="module")
def scen(pkg):
    return ss.scenarios(pkg)


def twin(pkg, receivers, capacity=1024, **kw):
    return pkg.capi.PositionTracker(capacity=capacity, receivers=receivers, host=True, table=True, sbs=True, **kw)


@pytest.mark.parametrize("name", ss.NAMES)
def test_scenario(pkg, scen, name):
    s = scen[name]
    m, f, r = ss.records(s["steps"])
    t = twin(pkg, s["receivers"], s["capacity"])
    if s["rows"] is None:
        pos, nic, trk = ss.run_library(t, s["steps"])
        mrows, mnic, model_rows = ss.run_model(s["receivers"], s["steps"])
        ss.same_rows(trk, model_rows)
        assert [(int(q["nic"]), int(q["rc"]), int(q["set"])) for q in nic] == mnic
    else:
        trk = s["rows"]
        model_rows = isbs.rows_of(trk)
    for opts, want in s["cases"]:
        got, ends = t.sbs_wire(m, f, trk, **opts)
        lines = ss.split(got, ends)
        model, mends = isbs.stream(m, f, model_rows, **opts)
        assert lines == want, [(i, a, b) for i, (a, b) in enumerate(zip(lines, want)) if a != b][:4]
        assert got == model and (ends == mends).all()
        assert max(len(x) for x in lines) <= pkg.capi.SBS_MAX
    t.close()


def test_mixed_stream(pkg):
    """2000 records of 40 aircraft: rows and text of the twin against the second reading, for every flag combination"""
    receivers, m, f, r = acs.mixed_stream(pkg)
    steps = [("update", m, f, r)]
    t = twin(pkg, receivers)
    pos, nic, trk = ss.run_library(t, steps)
    assert t.stats()["min_gate_margin_m"] >= 1.0
    _, _, model_rows = ss.run_model(receivers, steps)
    ss.same_rows(trk, model_rows)
    fl = trk["flags"]
    assert ((fl & isbs.TRACKED) == 0).sum() > 10 and (fl & isbs.CPR_DECODED).any() and (fl & isbs.GS_VALID).any()
    sizes = []
    for verbatim in (False, True):
        for net_only in (False, True):
            for gnss in (False, True):
                kw = dict(verbatim=verbatim, net_only=net_only, gnss=gnss, now_ms=ss.T0 + 5000, utc_offset_ms=7200000)
                got, ends = t.sbs_wire(m, f, trk, **kw)
                want, wends = isbs.stream(m, f, model_rows, **kw)
                assert got == want and (ends == wends).all()
                sizes.append(len(got))
    assert sizes[0] > 50000 and sizes[2] > sizes[0]
    # cut into calls, the rows are the same
    t2 = twin(pkg, receivers)
    assert ss.run_library(t2, steps, pieces=63)[2].tobytes() == trk.tobytes()
    t.close(), t2.close()


def test_other_update_calls_and_the_reducing_tracker(pkg, scen):
    """update_sbs on a tracker that reduces advances the timers as update_reduce does and can deliver the verdicts too;
    the other update calls keep working and change no row"""
    import reduce_streams as rs
    receivers, steps = rs.mixed_steps(pkg)
    a = twin(pkg, receivers, reduce_interval_ms=125)
    b = pkg.capi.PositionTracker(capacity=1024, receivers=receivers, host=True, table=True, reduce_interval_ms=125)
    plain = twin(pkg, receivers)
    calls = 0
    for s in steps:
        if s[0] == "expire":
            for t in (a, b, plain):
                t.expire(s[1])
            continue
        _, m, f, r = s
        want = plain.update_sbs(m, f, r)[3]
        fb = b.update_reduce(m, f, r)[2]
        if calls % 2:
            o, q, fa, trk = a.update_sbs(m, f, r, forward=True)
            assert fa.tobytes() == fb.tobytes() and trk.tobytes() == want.tobytes()
        else:
            a.update_nicrc(m, f, r)
        calls += 1
    with pytest.raises(pkg.MsdError) as e:  # verdicts from a tracker that does not reduce
        plain.update_sbs(m, f, r, forward=True)
    assert e.value.code == -errno.EINVAL
    for t in (a, b, plain):
        t.close()


def test_out_of_contract_values_stay_inside_the_longest_line(pkg):
    """what no decoder delivers is printed as an empty field: the line cannot outgrow MSD_SBS_MAX; and the longest line
    there is has exactly that length"""
    m = np.zeros(3, dtype=pkg.capi.MESSAGE_DTYPE)
    f = np.zeros(3, dtype=pkg.capi.FIELDS_DTYPE)
    trk = np.zeros(3, dtype=pkg.capi.SBS_TRACK_DTYPE)
    m["msgtype"], m["sysTimestampMsg"] = 20, ss.T0
    f["addr"] = 0xFFFFFF
    f["callsign_valid"], f["callsign"] = 1, b"WWWWWWWW"
    f["altitude_geom_valid"], f["altitude_geom"] = 1, -(1 << 31)
    f["geom_rate_valid"], f["geom_rate"] = 1, -32768
    f["squawk_valid"], f["squawk"], f["alert_valid"], f["alert"], f["spi_valid"], f["spi"], f["airground"] = 1, 0x7700, 1, 1, 1, 1, 1
    f["commb_format"], f["heading_valid"], f["heading_type"], f["heading_raw"] = 8, 1, 1, 2047
    trk["flags"] = isbs.TRACKED | isbs.SEEN_TWICE | isbs.GS_VALID | isbs.CPR_DECODED
    trk["gs_selected"], trk["lat"], trk["lon"] = [65535, 1e9, np.nan], [-180.0, 1e300, 360.5], [-180.0, 0, 0]
    t = twin(pkg, [None])
    got, ends = t.sbs_wire(m, f, trk, gnss=True, now_is_received=True)
    lines = ss.split(got, ends)
    assert lines[0] == (b"MSG,5,1,1,FFFFFF,1,2020/09/13,12:26:40.000,2020/09/13,12:26:40.000,WWWWWWWW,-2147483648H,65535,360,"
                        b"-180.00000,-180.00000,-32768H,7700,-1,-1,-1,-1\r\n")
    assert len(lines[0]) == pkg.capi.SBS_MAX == 147
    assert lines[1] == lines[2] == lines[0].replace(b",65535,360,-180.00000,-180.00000,", b",,360,,,")
    t.close()
