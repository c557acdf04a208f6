"""GPU checks of K36 through the C ABI: pvlm_refine_relative_poses against the host compile of the same core (tests/cpp/relpose_core_check.cpp) with the tolerances
of tests/test_relpose_cpu.py and equal step counts and termination codes (every scene here was held to the knife-edge condition there), bit-reproducibility, the
independence of a pair's result from its batch, the argument checks, and the chain behind pvlm_filter_image_pairs."""
import numpy as np
import pytest

from tests import essential_ref as er
from tests import relpose_ref as rr

pytestmark = pytest.mark.gpu

KINDS = ("pixel", "angle2")


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chk():
    return rr.build_check("off")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gpu(ctx, call, kind="pixel", max_num_iterations=50, check=True):
    from panovlm_amd import api
    g = api.refine_relative_poses(ctx, call["keypoints"], call["img_rows"], call["img_cols"], call["src"], call["tgt"], call["match_offsets"], call["matches"],
                                  call["inlier_offsets"], call["inlier_idx"], call["R_21"], call["t_21"], call["triangulated"], kind, max_num_iterations, check=check)
    assert g["guard_intact"]
    return g


def _against_host(g, h, call, kind):
    gp, hp = rr.split_points(g, call), rr.split_points(h, call)
    for p in range(len(call["src"])):
        s = h["summaries"][p]
        ref = dict(R_21=h["R_21"][p], t_21=h["t_21"][p], triangulated=hp[p], initial_cost=s["initial_cost"], final_cost=s["final_cost"], successful=s["successful_steps"],
                   unsuccessful=s["unsuccessful_steps"], termination=s["termination"], ok=h["ok"][p])
        print(p, tuple(g["summaries"][p]), tuple(s))
        rr.check_against(g, p, ref, gp[p], kind)


def _same_bits(a, b):
    for k in ("R_21", "t_21", "triangulated"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["ok"], b["ok"]) and np.array_equal(a["summaries"], b["summaries"])


def _size(label):
    from panovlm_amd import api
    W = api.relpose_workgroup_size()
    n = {"W-1": W - 1, "W": W, "W+1": W + 1, "4W+1": 4 * W + 1}.get(label)
    n = int(label) if n is None else n
    assert n in rr.SIZES, "a size whose scene the CPU tests did not hold to the knife-edge condition"
    return n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("label", ["0", "1", "2", "63", "64", "65", "W-1", "W", "W+1", "4W+1"])
def test_sizes_against_the_host_compile(ctx, chk, kind, label):
    """nothing, less than a lane's worth, both sides of the workgroup, a second, third, fourth and fifth trip of its loops"""
    n = _size(label)
    call = rr.assemble([rr.size_scene(n)])
    rc, h = rr.host_refine(chk, call, kind)
    assert rc == 0
    g = _gpu(ctx, call, kind)
    _against_host(g, h, call, kind)
    if n >= 8:
        assert g["summaries"]["successful_steps"][0] >= 2 and g["summaries"]["final_cost"][0] < g["summaries"]["initial_cost"][0]
    if n == 0:
        assert np.array_equal(_bits(g["R_21"]), _bits(call["R_21"])) and np.array_equal(_bits(g["t_21"]), _bits(call["t_21"])) and g["ok"][0] == 1


def _ragged():
    """0, 1, 65 and 300 inliers, the outlier scene, the pole scene; frame 1 is the target of the first pair and the source of the second"""
    scenes = [rr.size_scene(0), rr.size_scene(1), rr.size_scene(65), rr.size_scene(300), rr.outlier_scene(), rr.pole_scene()]
    return scenes, rr.assemble(scenes, [(0, 1), (1, 2), (3, 4), (5, 6), (7, 8), (9, 10)])


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch_three_ways(ctx, chk, kind, monkeypatch):
    scenes, call = _ragged()
    rc, h = rr.host_refine(chk, call, kind)
    assert rc == 0
    g = _gpu(ctx, call, kind)
    _against_host(g, h, call, kind)
    assert g["summaries"]["unsuccessful_steps"][4] >= 1                       # the outlier scene rejects steps on the device too
    _same_bits(_gpu(ctx, call, kind), g)                                      # two calls on the same input
    gp = rr.split_points(g, call)
    for p in range(len(scenes)):                                              # the per-pair calls
        one = _gpu(ctx, rr.subset(call, [p]), kind)
        assert np.array_equal(_bits(one["R_21"][0]), _bits(g["R_21"][p])) and np.array_equal(_bits(one["t_21"][0]), _bits(g["t_21"][p]))
        assert np.array_equal(_bits(one["triangulated"]), _bits(gp[p])) and one["ok"][0] == g["ok"][p] and one["summaries"][0] == g["summaries"][p]
    order = list(range(len(scenes)))[::-1]                                    # the pair list reversed
    back = _gpu(ctx, rr.subset(call, order), kind)
    bp = rr.split_points(back, rr.subset(call, order))
    for k, p in enumerate(order):
        assert np.array_equal(_bits(back["R_21"][k]), _bits(g["R_21"][p])) and np.array_equal(_bits(back["t_21"][k]), _bits(g["t_21"][p]))
        assert np.array_equal(_bits(bp[k]), _bits(gp[p])) and back["summaries"][k] == g["summaries"][p]
    monkeypatch.setenv("PVLM_RELPOSE_BATCH_PAIRS", "2")                        # the same list cut into three batches
    _same_bits(_gpu(ctx, call, kind), g)


def test_argument_errors_leave_the_outputs_untouched(ctx, chk):
    call = rr.assemble([rr.size_scene(8), rr.size_scene(65)])
    def refused(kind="pixel", it=50, **kw):
        c = dict(call); c.update(kw)
        g = _gpu(ctx, c, kind, it, check=False)
        assert g["rc"] == -1, g["rc"]
        assert np.array_equal(_bits(g["R_21"]), _bits(c["R_21"])) and np.array_equal(_bits(g["t_21"]), _bits(c["t_21"]))
        assert np.array_equal(_bits(g["triangulated"]), _bits(c["triangulated"])) and np.all(g["ok"] == 0xA5) and not g["summaries"]["termination"].any()
    idx = call["inlier_idx"].copy(); idx[70] = 65                             # pair 1 has 65 matches: 64 is its last
    refused(inlier_idx=idx)
    tri = call["triangulated"].copy(); tri[3, 2] = np.nan
    refused(triangulated=tri)
    refused(kind="angle1"); refused(it=-1)
    refused(tgt=np.array([1, 4], np.int32))
    R = call["R_21"].copy(); R[1, 0, 0] = np.inf
    refused(R_21=R)
    # max_num_iterations = 0: the input with the write-back applied, zero steps
    c = dict(call); c["t_21"] = call["t_21"] * 2.5
    z = _gpu(ctx, c, "pixel", 0)
    rc, h = rr.host_refine(chk, c, "pixel", 0)
    assert rc == 0 and not z["summaries"]["successful_steps"].any() and not z["summaries"]["unsuccessful_steps"].any()
    _against_host(z, h, c, "pixel")
    s = np.linalg.norm(c["t_21"], axis=1)
    assert np.abs(z["t_21"] - c["t_21"] / s[:, None]).max() <= 1e-15 and np.abs(z["R_21"] - c["R_21"]).max() <= 1e-15
    assert np.abs(z["triangulated"] - c["triangulated"] / np.repeat(s, [8, 65])[:, None]).max() <= 1e-14
    empty = _gpu(ctx, rr.subset(call, []), "pixel")
    assert len(empty["ok"]) == 0


def test_chain_behind_filter_image_pairs(ctx):
    """api.filter_image_pairs -> api.refine_relative_poses without reshaping: three frames, 30 % outlier matches, frame 1 in both pairs"""
    from panovlm_amd import api
    a1, a2, ma, _, Ra, ta = er.two_view_scene(np.random.default_rng(21), 200, 0.3)
    b1, b2, mb, _, Rb, tb = er.two_view_scene(np.random.default_rng(22), 200, 0.3, t=(0.3, 1.0, 0.2), w=(0.1, 0.05, -0.1))
    mb = mb.copy(); mb["query"] += len(a2)
    bearings = [a1, np.concatenate([a2, b1]), b2]
    off = np.array([0, 200, 400]); m = np.concatenate([ma, mb])
    gf = api.filter_image_pairs(ctx, bearings, [0, 1], [1, 2], off, m, 20, n_runs=6, max_iterations=100, seed=5)
    assert gf["keep"].tolist() == [1, 1] and gf["guard_intact"]
    kps = [rr.pixels_of(b) for b in bearings]
    g = api.refine_relative_poses(ctx, kps, [rr.ROWS] * 3, [rr.COLS] * 3, [0, 1], [1, 2], off, m, gf["offsets"], gf["inlier_idx"], gf["R_21"], gf["t_21"], gf["triangulated"])
    assert g["guard_intact"] and g["ok"].tolist() == [1, 1]
    print(g["summaries"])
    assert np.all(g["summaries"]["final_cost"] <= g["summaries"]["initial_cost"])
    for p, (R, t) in enumerate(((Ra, ta), (Rb, tb))):                         # K34's raw pose is fitted to every point it sampled, outliers included: the refinement improves it
        before = er.rotation_error_deg(gf["R_21"][p], R), er.direction_error_deg(gf["t_21"][p], t)
        after = er.rotation_error_deg(g["R_21"][p], R), er.direction_error_deg(g["t_21"][p], t)
        print(p, before, "->", after)
        assert after[0] < before[0] and after[1] < before[1]


def test_driver_chain_match_then_filter_full(tmp_path):
    """MatchImagePairs -> FilterImagePairsFull of the host mirror on a five-frame scene with depth maps: the same pairs in the same order as FilterImagePairsHost +
    RefineRelativePosesHost + the host tail, poses within 1e-6, the triangle survives the two bridges, the scale is the scene's (the driver checks all of it)"""
    import subprocess
    from panovlm_amd import build
    build.build_host()
    out = subprocess.run([build.RELPOSE_DRIVER, str(tmp_path / "pairs.txt")], capture_output=True, text=True, timeout=240)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(open(tmp_path / "pairs.txt").read().splitlines()) == 3
