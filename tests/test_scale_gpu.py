"""GPU checks of the resident depth maps (pvlm_depthset) and of K39 (pvlm_set_translation_scales) through the C ABI.  Depth sets: compute + read equals
pvlm_compute_depth_images on the same scans, also when the set is filled across three batches; upload + read round-trips; info of empty and mixed-size frames; a
closed set is refused.  Scales: the device equals the host compile of csrc/pvlm_scale_core.h (tests/cpp/scale_core_check.cpp) BIT FOR BIT -- the same IEEE fp64
operations in the same order, contraction off -- on a list that holds every scene of tests/test_scale_cpu.py, whatever the batch, the order or the neighbours.  The
chain: tests/cpp/pvlm_scale_driver.cpp prints equal RelativePair lists for the host-map route and the resident route."""
import subprocess

import numpy as np
import pytest

from tests import depthfill_ref as dref
from tests import scale_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def api():
    from panovlm_amd import api
    return api


# ---- depth sets -------------------------------------------------------------------------------------------------------------------------------
def test_depthset_compute_equals_compute_depth_images(ctx, api, monkeypatch):
    clouds = [dref.synthetic_cloud(3000, 1), dref.synthetic_cloud(2500, 2), np.zeros((0, 3), np.float32), dref.synthetic_cloud(4000, 4), dref.synthetic_cloud(1200, 5)]
    want, st0 = ctx.compute_depth_images(48, 96, clouds, dref.T_CL, 4, dref.MAX_DEPTH)
    assert want.any() and st0["batches"] == 1
    before = ctx.mem_info()
    for limit, batches in ((None, 1), ("2", 3)):
        if limit:
            monkeypatch.setenv("PVLM_DEPTHFILL_BATCH_IMAGES", limit)
        ds = api.DepthSet.compute(ctx, 48, 96, clouds, dref.T_CL, 4, dref.MAX_DEPTH)
        assert ds.stats["batches"] == batches and ds.stats["images"] == 5
        assert (ds.stats["valid_in"], ds.stats["valid_out"]) == (st0["valid_in"], st0["valid_out"])
        assert ctx.mem_info()["in_use"] >= before["in_use"] + 5 * 48 * 96 * 2       # the set is in use in the pool, as a DescSet is
        ctx.trim()                                                                # leaves a live set alone
        for f in range(5):
            assert ds.info(f) == (48, 96)
            assert np.array_equal(ds.read(f), want[f]), (limit, f)
        ds.close()
    assert ctx.mem_info()["in_use"] == before["in_use"]


def test_depthset_upload_read_info_and_use_after_close(ctx, api):
    rng = np.random.default_rng(3)
    ds = api.DepthSet.create(ctx, 4)
    a = rng.integers(0, 65536, size=(48, 96)).astype(np.uint16); b = rng.integers(0, 65536, size=(7, 13)).astype(np.uint16)
    ds.upload(0, a); ds.upload(2, b)
    assert [ds.info(f) for f in range(4)] == [(48, 96), (0, 0), (7, 13), (0, 0)]
    assert np.array_equal(ds.read(0), a) and np.array_equal(ds.read(2), b) and ds.read(1).shape == (0, 0)
    ds.upload(2, a[:5, :9])                                                       # a frame uploaded again takes the new map and size
    assert ds.info(2) == (5, 9) and np.array_equal(ds.read(2), a[:5, :9])
    with pytest.raises(api.PvlmError):
        ds.upload(4, a)
    with pytest.raises(api.PvlmError):
        ds.info(-1)
    rows = api.C.c_int(0); cols = api.C.c_int(0)
    assert ctx.lib.pvlm_depthset_read(ctx._h, ds._h, api.C.c_int(1), None) != 0       # an empty frame, a null target
    assert ctx.lib.pvlm_depthset_info(None, api.C.c_int(0), api.C.byref(rows), api.C.byref(cols)) != 0
    ds.close()
    for use in (lambda: ds.read(0), lambda: ds.info(0), lambda: ds.upload(0, a),
                lambda: api.set_translation_scales(ctx, ds, 96, 192, [96] * 4, [0], [2], [0, 0], np.eye(3), np.zeros(3), np.zeros((0, 3)))):
        with pytest.raises(api.PvlmError):
            use()
    ds.close()                                                                    # closing twice is harmless


# ---- scales ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return [sc for _, sc, _ in sr.all_scenes()]


@pytest.fixture(scope="module")
def host_results(scenes):
    """the host compile on every scene, computed once"""
    chk = sr.build_check()
    return [sr.host_core(chk, sc) for sc in scenes]


def _call(ctx, api, scenes, order):
    """one device call over scenes[order]: pair p reads frames 2 p and 2 p + 1 of a set made by create + upload (a missing map stays an empty frame)"""
    ds = api.DepthSet.create(ctx, 2 * len(order))
    frame_rows, off, R, t, X = [], [0], [], [], []
    for p, k in enumerate(order):
        sc = scenes[k]
        for j, d in enumerate((sc["d1"], sc["d2"])):
            if d is not None:
                ds.upload(2 * p + j, d)
        frame_rows += [sc["rows1"], sc["rows1"]]
        R.append(sc["R"]); t.append(sc["t"]); X.append(np.asarray(sc["X"], np.float64).reshape(-1, 3)); off.append(off[-1] + len(X[-1]))
    n = len(order)
    res = api.set_translation_scales(ctx, ds, sr.ROWS, sr.COLS, frame_rows, np.arange(n) * 2, np.arange(n) * 2 + 1, off, np.array(R), np.array(t), np.concatenate(X),
                                     points_with_depth=np.full(n, sr.START[0]), upper_scale=np.full(n, sr.START[1]), lower_scale=np.full(n, sr.START[2]))
    ds.close()
    return res, off


def _check(res, off, order, host_results):
    for p, k in enumerate(order):
        h = host_results[k]
        got = (res["ok"][p], res["t_21"][p], res["triangulated"][off[p]:off[p + 1]], res["points_with_depth"][p], res["upper_scale"][p], res["lower_scale"][p])
        assert res["ok"][p] in (0, 1)
        sr.same(got, h)
    st = res["stats"]
    exits = [host_results[k][6] for k in order]
    assert (st["pairs_mean"], st["pairs_median"], st["pairs_unscaled"]) == (exits.count("mean"), exits.count("median"), exits.count("none"))
    assert st["points_scaled"] == sum(host_results[k][7] for k in order)


def test_device_equals_host_compile(ctx, api, scenes, host_results, monkeypatch):
    n = len(scenes)
    assert 30 <= n <= 45 and api.scale_workgroup_size() == 64
    order = list(range(n))
    first, off = _call(ctx, api, scenes, order)
    assert first["stats"]["batches"] == 1
    _check(first, off, order, host_results)
    again, _ = _call(ctx, api, scenes, order)                                         # two runs: the same bits
    for key in ("t_21", "triangulated", "upper_scale", "lower_scale"):
        assert np.array_equal(sr.bits(first[key]), sr.bits(again[key])), key
    assert np.array_equal(first["ok"], again["ok"]) and np.array_equal(first["points_with_depth"], again["points_with_depth"])
    monkeypatch.setenv("PVLM_SCALE_BATCH_PAIRS", "7")                                # several batches, the last one short
    res, off = _call(ctx, api, scenes, order)
    assert res["stats"]["batches"] == (n + 6) // 7 and n % 7 != 0
    _check(res, off, order, host_results)
    rev = order[::-1]                                                                # other neighbours, other batches
    res, off = _call(ctx, api, scenes, rev)
    _check(res, off, rev, host_results)
    monkeypatch.delenv("PVLM_SCALE_BATCH_PAIRS")
    dup = order[:5] + [3] + order[5:]                                                # one pair twice
    res, off = _call(ctx, api, scenes, dup)
    _check(res, off, dup, host_results)


def test_argument_checks_leave_the_outputs(ctx, api, scenes):
    order = [1, 4]
    sc = [scenes[k] for k in order]
    ds = api.DepthSet.create(ctx, 4)
    for p, s in enumerate(sc):
        ds.upload(2 * p, s["d1"]); ds.upload(2 * p + 1, s["d2"])
    X = np.concatenate([np.asarray(s["X"], np.float64).reshape(-1, 3) for s in sc]); off = [0, len(sc[0]["X"]), len(X)]
    base = dict(eq_rows=sr.ROWS, eq_cols=sr.COLS, frame_rows=[sr.ROWS] * 4, src=[0, 2], tgt=[1, 3], point_offsets=off, R_21=np.array([s["R"] for s in sc]),
                t_21=np.array([s["t"] for s in sc]), triangulated=X)

    def rc_of(**kw):
        a = dict(base); a.update(kw)
        r = api.set_translation_scales(ctx, ds, check=False, points_with_depth=[3, 3], **a)
        if r["rc"] != 0:                                                           # refused: every output is as it came in
            assert np.array_equal(sr.bits(r["t_21"]), sr.bits(a["t_21"])) and np.array_equal(sr.bits(r["triangulated"]), sr.bits(a["triangulated"]))
            assert list(r["ok"]) == [0xA5, 0xA5] and list(r["points_with_depth"]) == [3, 3] and list(r["upper_scale"]) == [-1, -1] and list(r["lower_scale"]) == [-1, -1]
        return r["rc"]
    assert rc_of() == 0
    bad_t = base["t_21"].copy(); bad_t[1, 2] = np.inf
    bad_R = base["R_21"].copy(); bad_R[0, 1, 1] = np.nan
    bad_X = X.copy(); bad_X[3, 0] = np.nan
    ARG = -1
    assert rc_of(src=[0, 4]) == ARG and rc_of(tgt=[-1, 3]) == ARG
    assert rc_of(point_offsets=[1, off[1], off[2]]) == ARG and rc_of(point_offsets=[0, off[2], off[1]]) == ARG
    assert rc_of(t_21=bad_t) == ARG and rc_of(R_21=bad_R) == ARG and rc_of(triangulated=bad_X) == ARG
    assert rc_of(eq_rows=0) == ARG and rc_of(eq_cols=-3) == ARG
    ds.close()


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True])
def test_both_routes_give_the_same_pair_list(keep):
    """ComputeDepthImage + FilterImagePairsFull(DepthMaps) against ComputeDepthImageResident + FilterImagePairsFull(DeviceDepthMaps), through the driver, on the scene
    tests/test_depthfill_gpu.py uses"""
    from panovlm_amd import build
    out = subprocess.run([build.SCALE_DRIVER] + (["keep"] if keep else []), capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    a = [l.split("route", 1)[1] for l in out.stdout.splitlines() if l.startswith("host-map route")]
    b = [l.split("route", 1)[1] for l in out.stdout.splitlines() if l.startswith("resident route")]
    assert a == b and len(a) >= 4 and "resident maps equal host maps" in out.stdout
    assert "routes equal" in out.stdout and ("keep_no_scale %d" % keep) in out.stdout
