"""Session checkpoints when the two device logs behind them fill.

The reference-layout session snapshot reads two logs the kernels append to: the orphan log (PurgingTrigger with
allowed lateness: a purged session's cleanup timer outlives it) and the namespace log (an entry removed from a
"window-contents" namespace other keys still share).  Both hold max(64 Ki, 2 * max_batch) entries; FW_SESS_LOG_CAP
shrinks them so a few thousand records fill them.  Each log is pruned as the watermark advances, so what bounds it
is the entries a snapshot still needs, not the engine's lifetime; if those alone overflow it, snapshots fail with
FW_ERR_CAPACITY until the dropped entries no longer matter, and then succeed again, byte-identical.

Every comparison is against the oracle driven with the same stream and the same snapshot points: all 128 key
groups' state and timer bytes, and the fired epochs after the last snapshot.  fw_debug_session_logs (WindowEngine.
session_logs) guards each case: the log under test took at least 4 x its capacity in entries before the snapshot.
"""
import numpy as np
import pytest

from test_session_checkpoint import LONG_MAX, MP, _config, _diff, _epochs, _layout, _snap

CAP = 256
ORPHAN = ("i64", ("sum", "count"), 300, True)
ORPHAN_LONG = ("i64", ("sum", "count"), 5000, True)
NS_REDUCE = ("f64", ("sum", "min", "max", "count"), 400, False)
NS_LIST = ("f64", ("list",), 200, False)

# streams: records, keys, records per event-time second, timestamp grid, zipf exponent, records per push, and the
# number of key groups the keys are drawn from (default: all).  Timestamps snapped to the grid make many keys of a
# key group start sessions at one instant (shared namespaces); the pushes are short so that what one watermark
# appends to a 256-entry log fits beside what is still needed.  SHARED puts 2048 keys into two key groups, frequent
# ones (long sessions) beside rare ones: each key group then holds dozens of namespaces at a snapshot, many of them
# outliving the entry that created them, so that a namespace dated from a surviving entry instead of its logged
# first one changes the HashMap order (with the logs neither pruned nor checked, both cases differ from the oracle)
SMALL = dict(n=30_000, n_keys=2048, rate=384, grid=50, zipf=None, batch=48)
SHARED = dict(n=36_000, n_keys=2048, rate=384, grid=25, zipf=0.9, batch=48, kgs=2)
LARGE = dict(n=260_000, n_keys=4096, rate=1 << 12, grid=10, zipf=None, batch=512)

_streams = {}


def _stream(spec, vt):
    """The spec's stream, generated once per value type and shared (read-only) by the tests."""
    key = (tuple(sorted(spec.items(), key=str)), vt)
    if key not in _streams:
        from harness import gen_stream
        keys, ts, vals = gen_stream(spec["n"], spec["n_keys"], rate=spec["rate"], zipf=spec["zipf"], ooo=100,
                                    value_type=vt, seed=11)
        ts = ts // spec["grid"] * spec["grid"]
        if spec.get("kgs"):   # the keys drawn from the first `kgs` key groups only
            from flink_amd.keygroups import long_hash_code_np, murmur_hash_np
            cand = np.arange(1, 200 * spec["n_keys"], dtype=np.int64)
            keys = cand[murmur_hash_np(long_hash_code_np(cand)) % MP < spec["kgs"]][:spec["n_keys"]][keys]
        f1 = np.arange(len(keys), dtype=np.int64) * 7 + 3
        for a in (keys, ts, vals, f1):
            a.setflags(write=False)
        _streams[key] = (keys, ts, vals, f1)
    return _streams[key]


def _case_id(c):
    return f"{c[0]}-{'-'.join(c[1])}-late{c[2]}-{'purging' if c[3] else 'event'}"


def _run(factory, case, spec, restore=None, first_snapshot=True):
    """Drive to 1/3 (snapshot), to 2/3 (snapshot), then to the end and a final MAX_WATERMARK; with `restore` those
    sections are restored at the 2/3 watermark into a fresh engine, written back, and the last third driven.
    Returns (snapshots, outputs after the last snapshot, session_logs before each snapshot / fires up to it)."""
    from harness import drive
    vt, fields, lateness, purging = case
    keys, ts, vals, f1 = _stream(spec, vt)
    n1, n2, b = len(keys) // 3, 2 * len(keys) // 3, spec["batch"]
    wm2 = int(ts[:n2].max()) - 100
    layout = _layout(fields)
    e = factory(_config(vt, fields, lateness, purging))
    probe = (lambda: e.session_logs()) if e.prefix == "fw" else (lambda: e.stats()["panes_fired"])
    snaps, probes = [], []
    if restore is None:
        drive(e, keys[:n1], ts[:n1], vals[:n1], b, 100, None, f1=f1[:n1])
        probes.append(probe())
        if first_snapshot:
            snaps.append(_snap(e, layout))
        drive(e, keys[n1:n2], ts[n1:n2], vals[n1:n2], b, 100, None, f1=f1[n1:n2])
        e.advance_watermark(wm2)
        e.collect()
        probes.append(probe())
        snaps.append(_snap(e, layout))
    else:
        for kg, (st, tm) in restore.items():
            e.restore_kg_flink(kg, layout, st, tm, wm2)
        snaps.append(_snap(e, layout))
    out = drive(e, keys[n2:], ts[n2:], vals[n2:], b, 100, LONG_MAX, f1=f1[n2:])
    e.close()
    return snaps, out, probes


_oracle_runs = {}


def _oracle(case, spec):
    """The oracle's run of (case, spec), computed once."""
    from oracle.oracle import OracleEngine
    key = (case, tuple(sorted(spec.items(), key=str)))
    if key not in _oracle_runs:
        _oracle_runs[key] = _run(OracleEngine, case, spec)
    return _oracle_runs[key]


def _state_bytes(snap):
    return sum(len(st) for st, _ in snap.values())


def _orphans(snap, lateness):
    """Purged sessions' cleanup timers in a snapshot: under PurgingTrigger every in-flight window has both its
    timers, so the cleanup timers beyond the trigger timers belong to no window."""
    n = 0
    for _, tm in snap.values():
        cnt = int.from_bytes(tm[:4], "big", signed=True)
        t = np.frombuffer(tm, ">i8", 4 * cnt, 4).reshape(cnt, 4)
        n += int((t[:, 3] == t[:, 2] - 1 + lateness).sum()) - int((t[:, 3] == t[:, 2] - 1).sum())
    return n


# ---------------------------------------------------------------- CPU: the streams do what the GPU tests need


@pytest.mark.parametrize("case,spec,cap", [(ORPHAN, SMALL, CAP), (ORPHAN_LONG, SMALL, CAP), (NS_REDUCE, SHARED, CAP),
                                           (NS_LIST, SHARED, CAP), (ORPHAN, LARGE, 70_000 // 4)],
                         ids=["orphan-small", "orphan-long", "ns-reduce", "ns-list", "orphan-default-cap"])
def test_streams_fill_the_logs(case, spec, cap):
    """The oracle alone: between the two snapshot points more than 4 x cap sessions fire (the default-cap stream
    clears 70,000) and the second checkpoint holds in-flight sessions.  For the orphan ids that is the log's fill:
    each purged session is an entry.  For the namespace ids it shows only that the stream keeps sessions ending;
    that they leave namespaces still shared is not visible in the oracle, and rests on the GPU tests' own guard
    (namespace_appended) and on those tests failing without the pruning."""
    snaps, out, fired = _oracle(case, spec)
    assert fired[1] - fired[0] > 4 * cap, fired
    assert _state_bytes(snaps[-1]) > 8000
    assert sum(len(r) for _, r in _epochs(out, case)) > 1000
    if case == ORPHAN:        # few purged sessions' timers pending at once: the pruned log holds them
        assert 0 < _orphans(snaps[-1], case[2]) < (CAP if spec is SMALL else 65536) // 2, _orphans(snaps[-1], case[2])
    if case == ORPHAN_LONG:   # more pending at the 2/3 point than the small log holds
        assert _orphans(snaps[-1], case[2]) > 2 * CAP, _orphans(snaps[-1], case[2])


# ---------------------------------------------------------------- GPU: the HIP engine against the oracle


def _check_against_oracle(case, spec, log, cap):
    from flink_amd.windowing import WindowEngine
    from oracle.oracle import OracleEngine
    o, out_direct, _ = _oracle(case, spec)
    g, _, logs = _run(WindowEngine, case, spec)
    print(f"session logs before the snapshots: {logs}")
    assert logs[1][log + "_cap"] == cap
    assert logs[1][log + "_appended"] - logs[0][log + "_appended"] >= 4 * cap, logs
    assert _state_bytes(o[-1]) > 8000
    for i in range(len(o)):
        assert _diff(g[i], o[i]) is None, (i, _diff(g[i], o[i]))
    back, out_g, _ = _run(WindowEngine, case, spec, restore=o[-1])
    _, out_o, _ = _run(OracleEngine, case, spec, restore=o[-1])
    assert _diff(back[0], o[-1]) is None, _diff(back[0], o[-1])
    eg, eo = _epochs(out_g, case), _epochs(out_o, case)
    assert eg == eo and eo == _epochs(out_direct, case) and sum(len(r) for _, r in eo) > 1000


@pytest.mark.gpu
def test_orphan_log_small_cap(monkeypatch):
    """More than 4 x 256 sessions purge between the snapshots, most of their cleanup timers long fired: the log is
    pruned as the watermark advances, the second snapshot succeeds and is the oracle's, and the oracle's bytes
    restore, write back unchanged and continue like the oracle."""
    monkeypatch.setenv("FW_SESS_LOG_CAP", str(CAP))
    _check_against_oracle(ORPHAN, SMALL, "orphan", CAP)


@pytest.mark.gpu
def test_orphan_log_recoverable_overflow(monkeypatch):
    """Lateness 5000: more than 256 purged sessions' timers are pending at once, the log drops some, and the
    snapshot at 2/3 fails with FW_ERR_CAPACITY instead of leaving their timers out.  Once the watermark has passed
    the dropped timers a snapshot succeeds again and is the oracle's; the fires of the whole run are the oracle's."""
    from flink_amd import _abi
    from flink_amd.windowing import WindowEngine
    from harness import drive
    from oracle.oracle import OracleEngine
    monkeypatch.setenv("FW_SESS_LOG_CAP", str(CAP))
    case = ORPHAN_LONG
    vt, fields, lateness, purging = case
    keys, ts, vals, f1 = _stream(SMALL, vt)
    n2, b = 2 * len(keys) // 3, SMALL["batch"]
    layout = _layout(fields)
    end = int(ts.max())
    wm_after = end + lateness + 1000                 # past every timer of the stream, well short of MAX_WATERMARK
    nf = 400                                          # fresh records, a key each: sessions in flight at the last snapshot
    fk = np.arange(nf, dtype=np.int64) * 31 + 5
    fts = wm_after + 200 + (np.arange(nf, dtype=np.int64) % 4) * 50
    fv = np.arange(nf, dtype=np.int64)
    res = {}
    for name, factory in (("g", WindowEngine), ("o", OracleEngine)):
        e = factory(_config(vt, fields, lateness, purging))
        out = drive(e, keys[:n2], ts[:n2], vals[:n2], b, 100, None, f1=f1[:n2])
        if name == "g":
            logs = e.session_logs()
            print(f"session logs at 2/3: {logs}")
            assert logs["orphan_cap"] == CAP and logs["orphan_appended"] >= 4 * CAP and logs["lossy"] == 1, logs
            with pytest.raises(_abi.FwError) as ei:
                _snap(e, layout)
            assert ei.value.code == _abi.FW_ERR_CAPACITY
        out += drive(e, keys[n2:], ts[n2:], vals[n2:], b, 100, wm_after, f1=f1[n2:])
        out += drive(e, fk, fts, fv, nf, 100, None, f1=fv)
        if name == "g":
            assert e.session_logs()["lossy"] == 0
        snap = _snap(e, layout)
        e.advance_watermark(LONG_MAX)
        out.append(e.collect())
        e.close()
        res[name] = (snap, _epochs(out, case))
    assert _state_bytes(res["o"][0]) > 8000, "the snapshot after the recovery holds in-flight sessions"
    assert _diff(res["g"][0], res["o"][0]) is None, _diff(res["g"][0], res["o"][0])
    assert res["g"][1] == res["o"][1] and sum(len(r) for _, r in res["o"][1]) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("case", [NS_REDUCE, NS_LIST], ids=_case_id)
def test_namespace_log_small_cap(case, monkeypatch):
    """More than 4 x 256 entries leave namespaces other keys still share; the pruned log keeps the ones whose
    namespace is still live, and both snapshots order the namespaces as the oracle's HashMap does."""
    monkeypatch.setenv("FW_SESS_LOG_CAP", str(CAP))
    _check_against_oracle(case, SHARED, "namespace", CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("case,spec,log", [(ORPHAN, SMALL, "orphan"), (NS_REDUCE, SHARED, "namespace")],
                         ids=["orphan", "namespace"])
def test_small_cap_hot_walk(case, spec, log, monkeypatch):
    """The same with FW_SESS_HOT=4: k_sess_walk_hot appends to the same logs."""
    monkeypatch.setenv("FW_SESS_LOG_CAP", str(CAP))
    monkeypatch.setenv("FW_SESS_HOT", "4")
    _check_against_oracle(case, spec, log, CAP)


@pytest.mark.gpu
def test_orphan_log_default_cap():
    """No override (65,536 entries): more than 70,000 sessions purge between the snapshots and the second snapshot
    is the oracle's."""
    from flink_amd.windowing import WindowEngine
    o, _, fired = _oracle(ORPHAN, LARGE)
    g, _, logs = _run(WindowEngine, ORPHAN, LARGE)
    print(f"session logs before the snapshots: {logs}")
    assert logs[1]["orphan_cap"] == 65536
    assert logs[1]["orphan_appended"] - logs[0]["orphan_appended"] > 70_000, logs
    assert _state_bytes(o[-1]) > 8000
    for i in range(len(o)):
        assert _diff(g[i], o[i]) is None, (i, _diff(g[i], o[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [NS_REDUCE, ORPHAN], ids=_case_id)
def test_advance_list_stays_short(case):
    """The host's list of watermark advances exists for restored purged sessions' timers only: without a restore
    200 advances leave it at one entry at most."""
    from flink_amd.windowing import WindowEngine
    from harness import drive
    vt, fields, lateness, purging = case
    keys, ts, vals, f1 = _stream(SMALL, vt)
    e = WindowEngine(_config(vt, fields, lateness, purging))
    n = 200 * SMALL["batch"]
    drive(e, keys[:n], ts[:n], vals[:n], SMALL["batch"], 100, None, f1=f1[:n])
    assert e.session_logs()["advances"] <= 1
    e.close()


@pytest.mark.gpu
def test_advance_list_after_restore():
    """Restored with purged sessions' timers pending, the list grows while they are, and is back at one entry once
    the watermark has passed the last of them."""
    from flink_amd.windowing import WindowEngine
    from harness import drive
    case = ORPHAN
    vt, fields, lateness, purging = case
    o, _, _ = _oracle(case, SMALL)
    keys, ts, vals, f1 = _stream(SMALL, vt)
    n2, b = 2 * len(keys) // 3, SMALL["batch"]
    wm2 = int(ts[:n2].max()) - 100
    assert _orphans(o[-1], lateness) > 0
    e = WindowEngine(_config(vt, fields, lateness, purging))
    for kg, (st, tm) in o[-1].items():
        e.restore_kg_flink(kg, _layout(fields), st, tm, wm2)
    sl = slice(n2, n2 + b)
    e.push(keys[sl], ts[sl], vals[sl], f1=f1[sl])
    e.advance_watermark(wm2 + 20)   # short of the restored timers of sessions that ended just before the checkpoint
    assert e.session_logs()["advances"] == 2, e.session_logs()
    sl = slice(n2 + b, n2 + 20 * b)
    drive(e, keys[sl], ts[sl], vals[sl], b, 100, None, f1=f1[sl])
    assert int(ts[sl].max()) - 100 > wm2 + 150 + lateness
    assert e.session_logs()["advances"] <= 1
    e.close()
