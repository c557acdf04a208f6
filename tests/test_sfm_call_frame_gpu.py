"""What the call frame of the SfM stages (panovlm_amd/csrc/pvlm_call.h, K31-K37) guarantees and no other test looks at: every entry point gives its device scratch back
on every way out, a refused call leaves nothing behind that could change the next one (no staged copy, no stale launch error), a graph capture is refused by all of them
in the same way, and the batch limits read from the environment fall back to the built-in limit for anything that is not a smaller positive number.  The inputs are the
existing generators at their smallest sizes; the results themselves are checked against the host compiles elsewhere, here only against a repeat of the same call."""
import re

import numpy as np
import pytest

from tests import depthfill_ref as dr
from tests import essential_ref as er
from tests import match_ref as mr
from tests import relpose_ref as rr
from tests import structure_ref as sr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_CAPACITY = -1, -4, -5
ESS = dict(n_runs=4, max_iterations=60, seed=5)


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """3 frames of 40-70 descriptors, 3 pairs of about 60 matches, 2 images of 24 x 40, 12 tracks"""
    rng = np.random.default_rng(3700)
    A, B, _ = mr.float_descriptors(rng, 55, 70)
    d = dict(frames=[A, B, mr.float_descriptors(rng, 40, 70)[0]], src=np.array([0, 0, 2], np.int32), tgt=np.array([1, 2, 1], np.int32))
    scenes = [er.two_view_scene(rng, n) for n in (60, 57, 64)]
    d["bearings"] = [b for s in scenes for b in s[:2]]
    d["e_src"] = np.array([0, 2, 4], np.int32); d["e_tgt"] = np.array([1, 3, 5], np.int32)
    d["e_matches"] = np.concatenate([s[2] for s in scenes]); d["e_off"] = np.array([0, 60, 117, 181], np.int64)
    d["relpose"] = rr.assemble([rr.pair_scene(900 + n, n) for n in (60, 57, 64)])
    tr = sr.random_tracks(rng, 12, 5, [2, 3, 4])
    tr["kp"] = rr.pixels_of(tr["b"])
    d["tracks"] = tr
    d["sparse"] = np.stack([dr.recipe(24, 40, 0.2, seed=s) for s in (1, 2)])
    d["clouds"] = [dr.synthetic_cloud(n, s) for n, s in ((300, 1), (250, 2))]
    return d


def _freeze(x, drop=()):
    """A result as something == compares byte for byte: arrays by dtype, shape and bytes (records field by field: their padding is nobody's result); the times of the
    statistics, and the keys in `drop`, left out."""
    if isinstance(x, np.ndarray):
        if x.dtype.names:
            return tuple((n, _freeze(np.ascontiguousarray(x[n]))) for n in x.dtype.names)
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, _freeze(v, drop)) for k, v in sorted(x.items()) if not k.endswith("_ms") and k not in drop)
    if isinstance(x, (tuple, list)):
        return tuple(_freeze(v, drop) for v in x)
    return x


def _status(call):
    """The pvlm_status a call ends with: parsed from the PvlmError as Context._check formats it; the wrappers with a capacity report -5 as overflow."""
    import panovlm_amd as pv
    try:
        r = call()
    except pv.PvlmError as e:
        m = re.search(r"failed \((-?\d+)\)", str(e))
        assert m, str(e)
        return int(m.group(1))
    if isinstance(r, dict) and r.get("overflow"):
        return ERR_CAPACITY
    return int(r["rc"]) if isinstance(r, dict) and "rc" in r else 0


def _with(arr, at, value):
    out = np.array(arr, copy=True)
    out[at] = value
    return out


def _descset(ctx, frames):
    import panovlm_amd as pv
    ds = pv.api.DescSet(ctx, frames)
    rows = ds.rows.copy()
    ds.close()
    return rows


def _embed(ctx, ds, cb, alive):
    import panovlm_amd as pv
    vs = pv.api.vlad_embed(ctx, ds, cb, alive, 2)
    try:
        nb, sim = pv.api.vlad_neighbors(ctx, vs, 2, want_sim=True)
        return vs.read(), vs.stats, nb, sim
    finally:
        vs.close()


def _cases(ctx, d, ds):
    """name -> (the successful call, [(a call that is refused, its status)]); ds: the descriptor set of d["frames"], which the caller keeps open"""
    import panovlm_amd as pv
    api = pv.api
    t = d["tracks"]; rp = d["relpose"]; n_obs = len(t["fid"])
    bad_fid = _with(t["fid"], n_obs - 1, 5)
    bad_tgt = _with(d["tgt"], 1, 3)                  # the wrappers size their outputs by the src frames' rows: the frame that is not there is a tgt
    bad_esrc = _with(d["e_src"], 2, 6)
    init = np.array([3, 60, 120, 90], np.int64)
    cb, alive = api.vlad_kmeans(ctx, ds, [0, 1, 2], 4, 3, init)[:2]
    ess = lambda f, **kw: f(ctx, d["bearings"], kw.pop("src", d["e_src"]), d["e_tgt"], d["e_off"], d["e_matches"], **kw, **ESS)
    depth = d["sparse"]
    first = np.array([0, 300, 550], np.int64); xyz = np.concatenate(d["clouds"])
    return (cb, alive), {
        "filter_tracks": (lambda: api.filter_tracks(ctx, "angle", 720, 1440, t["off"], t["fid"], t["kp"], t["X"], t["T"], 2.0),
                          [(lambda: api.filter_tracks(ctx, "angle", 720, 1440, t["off"], bad_fid, t["kp"], t["X"], t["T"], 2.0), ERR_ARG)]),
        "triangulate_tracks": (lambda: api.triangulate_tracks(ctx, 0, 0, t["off"], t["fid"], t["T"], bearings=t["b"]),
                               [(lambda: api.triangulate_tracks(ctx, 0, 0, t["off"], bad_fid, t["T"], bearings=t["b"]), ERR_ARG)]),
        "filter_tracks_far": (lambda: api.filter_tracks_far(ctx, t["off"], t["fid"], t["X"], t["centres"], 3.0),
                              [(lambda: api.filter_tracks_far(ctx, t["off"], bad_fid, t["X"], t["centres"], 3.0), ERR_ARG)]),
        "descset_create": (lambda: _descset(ctx, d["frames"]),
                           [(lambda: _descset(ctx, [d["frames"][0], _with(d["frames"][1], (69, 127), np.nan), d["frames"][2]]), ERR_ARG)]),
        "match_knn2": (lambda: api.match_knn2(ctx, ds, d["src"], d["tgt"]), [(lambda: api.match_knn2(ctx, ds, d["src"], bad_tgt), ERR_ARG)]),
        "match_pairs": (lambda: api.match_pairs(ctx, ds, d["src"], d["tgt"], 0.8, 0),
                        [(lambda: api.match_pairs(ctx, ds, d["src"], bad_tgt, 0.8, 0), ERR_ARG), (lambda: api.match_pairs(ctx, ds, d["src"], d["tgt"], 0.8, 0, capacity=1), ERR_CAPACITY)]),
        "essential_acransac": (lambda: ess(api.essential_acransac), [(lambda: ess(api.essential_acransac, src=bad_esrc), ERR_ARG), (lambda: ess(api.essential_acransac, capacity=1), ERR_CAPACITY)]),
        "filter_image_pairs": (lambda: ess(api.filter_image_pairs, triangulation_num_threshold=10),
                               [(lambda: ess(api.filter_image_pairs, triangulation_num_threshold=10, src=bad_esrc), ERR_ARG),
                                (lambda: ess(api.filter_image_pairs, triangulation_num_threshold=10, capacity=1), ERR_CAPACITY)]),
        "vlad_kmeans": (lambda: api.vlad_kmeans(ctx, ds, [0, 1, 2], 4, 3, init), [(lambda: api.vlad_kmeans(ctx, ds, [0, 3, 2], 4, 3, init), ERR_ARG)]),
        "vlad_embed_read_neighbors": (lambda: _embed(ctx, ds, cb, alive), [(lambda: _embed(ctx, ds, _with(cb, (1, 7), np.inf), None), ERR_ARG)]),
        "refine_relative_poses": (lambda: api.refine_relative_poses(ctx, **rp, max_num_iterations=5),
                                  [(lambda: api.refine_relative_poses(ctx, **dict(rp, tgt=_with(rp["tgt"], 0, 6)), max_num_iterations=5), ERR_ARG)]),
        "depth_completion": (lambda: ctx.depth_completion(depth, dr.MAX_DEPTH, want_f32=True, want_u16=True),
                             [(lambda: ctx.depth_completion(_with(dr.as_f32(depth), (1, 23, 39), -1.0), dr.MAX_DEPTH), ERR_ARG)]),
        "compute_depth_images": (lambda: ctx.compute_depth_images_flat(24, 40, first, xyz, dr.T_CL, 3, dr.MAX_DEPTH),
                                 [(lambda: ctx.compute_depth_images_flat(24, 40, _with(first, 1, 600), xyz, dr.T_CL, 3, dr.MAX_DEPTH), ERR_ARG)]),
    }


NAMES = ["filter_tracks", "triangulate_tracks", "filter_tracks_far", "descset_create", "match_knn2", "match_pairs", "essential_acransac", "filter_image_pairs", "vlad_kmeans",
         "vlad_embed_read_neighbors", "refine_relative_poses", "depth_completion", "compute_depth_images"]


@pytest.fixture(scope="module")
def cases(ctx, data):
    import panovlm_amd as pv
    ds = pv.api.DescSet(ctx, data["frames"])
    book, c = _cases(ctx, data, ds)
    assert sorted(c) == sorted(NAMES)
    for ok, _ in c.values():            # the warm calls: the pool has its slabs, the code objects are loaded
        ok()
    c["_vladset_inputs"] = (ds,) + book
    yield c
    ds.close()


@pytest.fixture(scope="module")
def first_results(cases):
    """The result of the first successful call of every case (after the warm one), frozen: what every later repeat must equal byte for byte."""
    return {name: _freeze(cases[name][0]()) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_scratch_goes_back_and_a_refused_call_leaves_nothing_behind(ctx, cases, first_results, name):
    ok, refused = cases[name]
    in_use = ctx.mem_info()["in_use"]
    assert _freeze(ok()) == first_results[name]
    assert ctx.mem_info()["in_use"] == in_use
    for call, status in refused:
        assert _status(call) == status
        assert ctx.mem_info()["in_use"] == in_use, status
        assert _freeze(ok()) == first_results[name], status          # no staged copy and no launch error survived the refused call
        assert ctx.mem_info()["in_use"] == in_use, status


def test_capacity_error_still_reports_the_whole_result(cases, first_results):
    """PVLM_ERR_CAPACITY of the three entry points with a capacity: needed, keep and the offsets are those of the full call, the records stop at the capacity."""
    for name, records in (("match_pairs", "matches"), ("essential_acransac", "inliers"), ("filter_image_pairs", "inlier_idx")):
        full = cases[name][0]()
        short = cases[name][1][1][0]()
        assert short["overflow"] and short["guard_intact"] and short["needed"] == full["needed"] > 1
        assert np.array_equal(short["offsets"], full["offsets"]) and len(short[records]) == 1 and short[records][0] == full[records][0]
        if "keep" in full:
            assert np.array_equal(short["keep"], full["keep"])


def test_a_graph_capture_is_refused_by_every_entry_point(ctx, cases, first_results):
    """Between graph_begin and graph_end every entry point ends with PVLM_ERR_STATE before it allocates, copies or launches; the capture (one capturable call is recorded
    in it, so that it is not empty) can still be ended, and the calls after it give the results from before."""
    import torch
    import panovlm_amd as pv
    dev = torch.device("cuda", 0)
    cam = torch.randn((64, 3), dtype=torch.float32).to(dev); px = torch.empty((64, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ds, cb, alive = cases["_vladset_inputs"]
    vs = pv.api.vlad_embed(ctx, ds, cb, alive, 2)                    # pvlm_vladset_read and pvlm_vlad_neighbors need a set from before the capture
    try:
        in_use = ctx.mem_info()["in_use"]
        ctx.graph_begin()
        try:
            ctx.cam_to_image_f32_dev(720, 1440, 64, cam.data_ptr(), px.data_ptr())
            status = {name: _status(cases[name][0]) for name in NAMES}
            status["vladset_read"] = _status(vs.read)
            status["vlad_neighbors"] = _status(lambda: pv.api.vlad_neighbors(ctx, vs, 2))
        finally:
            g = ctx.graph_end()
        g.close()
        assert status == {name: ERR_STATE for name in NAMES + ["vladset_read", "vlad_neighbors"]}
        assert ctx.mem_info()["in_use"] == in_use
    finally:
        vs.close()
    for name in NAMES:
        assert _freeze(cases[name][0]()) == first_results[name], name


LIMITS = {"match": ("PVLM_MATCH_BATCH_QUERIES", "match_pairs", "60", lambda r: r["stats"]["batches"]),
          "vlad": ("PVLM_VLAD_BATCH_ROWS", "vlad_kmeans", "60", lambda r: r[3]["batches"]),
          "depthfill": ("PVLM_DEPTHFILL_BATCH_IMAGES", "depth_completion", "1", lambda r: r[2]["batches"])}


@pytest.mark.parametrize("stage", sorted(LIMITS))
def test_batch_limit_from_the_environment(cases, first_results, monkeypatch, stage):
    """pvlm_i_env_limit: 0, a negative number, text and a value above the built-in limit leave the limit alone (same results, same number of batches); a small value
    gives more batches and the same bytes.  The other two variables (essential, relpose) report no batch count; test_essential_gpu.py and test_relpose_gpu.py cover them."""
    var, name, small, batches = LIMITS[stage]
    ok = cases[name][0]
    monkeypatch.delenv(var, raising=False)
    unset = ok()
    assert _freeze(unset) == first_results[name]
    for value in ("0", "-3", "abc", str(1 << 40)):
        monkeypatch.setenv(var, value)
        assert _freeze(ok()) == first_results[name], value
    monkeypatch.setenv(var, small)
    r = ok()
    assert batches(r) > batches(unset)
    assert _freeze(r, drop=("batches",)) == _freeze(unset, drop=("batches",))
