"""Builds libpvlm.so (HIP kernels + C ABI, gfx950) in-tree with hipcc.  No JIT cache: the .so sits
next to this file so that it travels to the GPU box with the repo snapshot."""
import glob
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpvlm.so")
ARCH = "gfx950"
# sources whose float / double decisions must equal a non-FMA x86-64 build of the reference bit for bit
NO_CONTRACT = ("pvlm_assoc.hip", "pvlm_lines.hip", "pvlm_linegrow.hip", "pvlm_mvs.hip", "pvlm_ring.hip", "pvlm_undistort.hip", "pvlm_fuse.hip", "pvlm_texture.hip",
               "pvlm_sfm_filter.hip", "pvlm_triangulate.hip", "pvlm_match.hip", "pvlm_essential.hip", "pvlm_vlad.hip", "pvlm_depthfill.hip", "pvlm_scale.hip", "pvlm_sift.hip", "pvlm_transavg.hip", "pvlm_rotavg.hip", "pvlm_bata.hip", "pvlm_rotstart.hip", "pvlm_transdir.hip", "pvlm_translp.hip", "pvlm_triplet.hip", "pvlm_neighbor_sfm.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm >= 7.0 for gfx950)")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "pvlm.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    objs = []
    bdir = os.path.join(HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    common = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
    procs = []
    for src in sources():
        obj = os.path.join(bdir, os.path.basename(src) + ".o")
        flags = list(common) + os.environ.get("PVLM_DEFINES", "").split()
        # association kernels make accept/reject decisions that must be bit-identical to a
        # non-FMA x86-64 build of the reference: no contraction there.
        if os.path.basename(src) in NO_CONTRACT:
            flags.append("-ffp-contract=off")
        # the candidate loop of the k-NN search: SLP packs two of its three float subtractions / multiplications into v_pk ops and pays
        # three register moves to assemble the operands — measured 2 % slower than the scalar form (23.6 vs 23.15 ms per 134 M queries)
        if os.path.basename(src) == "pvlm_assoc.hip":
            flags.append("-fno-slp-vectorize")
        cmd = [_hipcc()] + flags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out)
            raise RuntimeError("hipcc failed on " + src)
        if verbose and out.strip():
            print(out)
    cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl", "-pthread"]
    subprocess.check_call(cmd)
    return LIB


def build_variant(tag, defines):
    """A measured variant of the library: build/var/libpvlm_<tag>.so with extra -D switches (e.g. ["-DPVLM_NT_LOADS=0"]), selected at
    run time through PVLM_LIB (tools/ab_eval_loads.sh).  A source is recompiled when it, or any header under csrc/, mentions one of
    the switches (a switch consumed in a header reaches every source that may include it); the other objects are those of the
    in-tree build.  Same flags as the in-tree build (PVLM_DEFINES included).  A switch nobody mentions is an error: the variant
    would silently equal the baseline.  python -m panovlm_amd.build --variant temporal -DPVLM_NT_LOADS=0"""
    build(force=False)
    vdir = os.path.join(HERE, "..", "build", "var")
    os.makedirs(vdir, exist_ok=True)
    names = [d[2:].split("=")[0] for d in defines if d.startswith("-D")]
    headers = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith(".h")}
    in_header = [n for n in names if any(n in t for t in headers.values())]
    mentioned = set(in_header)
    objs = []
    for src in sources():
        base = os.path.basename(src)
        obj = os.path.join(HERE, "build", base + ".o")
        text = open(src).read()
        mentioned.update(n for n in names if n in text)
        if any(n in text for n in names) or in_header:
            obj = os.path.join(vdir, base + "." + tag + ".o")
            flags = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
            flags += os.environ.get("PVLM_DEFINES", "").split() + list(defines)
            if base in NO_CONTRACT:
                flags.append("-ffp-contract=off")
            if base == "pvlm_assoc.hip":
                flags.append("-fno-slp-vectorize")
            subprocess.check_call([_hipcc()] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    missing = [n for n in names if n not in mentioned]
    if missing:
        raise RuntimeError("no source or header under csrc/ mentions %s: the variant would equal the baseline" % ", ".join(missing))
    out = os.path.join(vdir, "libpvlm_%s.so" % tag)
    subprocess.check_call([_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", out] + objs + ["-ldl", "-pthread"])
    return out


HOST_LIB = os.path.join(HERE, "libpvlm_host.so")
HOST_DRIVER = os.path.join(HERE, "build", "pvlm_host_driver")
FUSE_DRIVER = os.path.join(HERE, "build", "pvlm_fuse_driver")
TEXTURE_DRIVER = os.path.join(HERE, "build", "pvlm_texture_driver")
SFM_DRIVER = os.path.join(HERE, "build", "pvlm_sfm_driver")
STRUCTURE_DRIVER = os.path.join(HERE, "build", "pvlm_structure_driver")
MATCH_DRIVER = os.path.join(HERE, "build", "pvlm_match_driver")
ESSENTIAL_DRIVER = os.path.join(HERE, "build", "pvlm_essential_driver")
VLAD_DRIVER = os.path.join(HERE, "build", "pvlm_vlad_driver")
RELPOSE_DRIVER = os.path.join(HERE, "build", "pvlm_relpose_driver")
DEPTHFILL_DRIVER = os.path.join(HERE, "build", "pvlm_depthfill_driver")
DEPTHFILL_CHECK = os.path.join(HERE, "build", "depthfill_core_check")
SCALE_DRIVER = os.path.join(HERE, "build", "pvlm_scale_driver")
DISPATCH_ORDER_CHECK = os.path.join(HERE, "build", "dispatch_order_check")
SIFT_DRIVER = os.path.join(HERE, "build", "pvlm_sift_driver")
TRANSAVG_DRIVER = os.path.join(HERE, "build", "pvlm_transavg_driver")
ROTAVG_DRIVER = os.path.join(HERE, "build", "pvlm_rotavg_driver")
BATA_DRIVER = os.path.join(HERE, "build", "pvlm_bata_driver")
ROTSTART_DRIVER = os.path.join(HERE, "build", "pvlm_rotstart_driver")
TRANSDIR_DRIVER = os.path.join(HERE, "build", "pvlm_transdir_driver")
TRANSLP_DRIVER = os.path.join(HERE, "build", "pvlm_translp_driver")
TRIPLET_DRIVER = os.path.join(HERE, "build", "pvlm_triplet_driver")
NEIGHBOR_DRIVER = os.path.join(HERE, "build", "pvlm_neighbor_driver")


def build_host(force=False):
    """libpvlm_host.so (C++ mirror of PanoVLM's interfaces above the C ABI) and its test driver."""
    build(force=False)
    hdir = os.path.join(HERE, "host")
    # one translation unit per mirrored reference file (pvlm_host_*.cpp), the feature extractor (pvlm_features.cpp, pvlm_lines.cpp) and the
    # core (pvlm_host.cpp); -ffp-contract=off everywhere: the float threshold decisions of the extractor and the double chains of the
    # solver must not pick up FMAs the oracle does not have
    srcs = sorted(glob.glob(os.path.join(hdir, "*.cpp")))
    hdrs = sorted(glob.glob(os.path.join(hdir, "*.hpp"))) + [os.path.join(HERE, "csrc", "pvlm_workers.h"), os.path.join(HERE, "..", "include", "pvlm.h")]
    drv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_host_driver.cpp")
    odir = os.path.join(HERE, "build", "host")
    os.makedirs(odir, exist_ok=True)
    newest_hdr = max(os.path.getmtime(x) for x in hdrs)
    objs, jobs = [], []
    for s in srcs:
        o = os.path.join(odir, os.path.basename(s)[:-4] + ".o")
        objs.append(o)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(s), newest_hdr):
            jobs.append(["g++", "-std=c++17", "-O2", "-fPIC", "-Wall", "-ffp-contract=off", "-c", s, "-o", o])
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as pool:
            list(pool.map(subprocess.check_call, jobs))
    if jobs or not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < os.path.getmtime(LIB):
        subprocess.check_call(["g++", "-shared", "-o", HOST_LIB] + objs + ["-L" + HERE, "-lpvlm", "-pthread", "-Wl,-rpath,$ORIGIN"])
    adapter = os.path.join(HERE, "..", "integration", "pvlm_ceres.hpp")
    if os.path.exists(drv) and (force or not os.path.exists(HOST_DRIVER) or
                                os.path.getmtime(HOST_DRIVER) < max(os.path.getmtime(drv), os.path.getmtime(HOST_LIB), os.path.getmtime(adapter))):
        root = os.path.join(HERE, "..")
        # integration/pvlm_ceres.hpp is compiled into the driver against tests/cpp/ceres_double: an interface-only stand-in
        # for the handful of Ceres classes the adapter touches (this image has no Ceres)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "tests", "cpp", "ceres_double"),
                               drv, "-o", HOST_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm", "-Wl,-rpath," + HERE])
    # the fused map's driver (FuseLidar, SavePCDFileBinary, the timing of the device call against the host loop)
    fdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_fuse_driver.cpp")
    if os.path.exists(fdrv) and (force or not os.path.exists(FUSE_DRIVER) or
                                 os.path.getmtime(FUSE_DRIVER) < max(os.path.getmtime(fdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", fdrv, "-o", FUSE_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the coloured map's driver (Texture, SegmentBatch, SavePCDFileBinary of PointXYZRGB, the timing of the device call against the host loop)
    tdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_texture_driver.cpp")
    if os.path.exists(tdrv) and (force or not os.path.exists(TEXTURE_DRIVER) or
                                 os.path.getmtime(TEXTURE_DRIVER) < max(os.path.getmtime(tdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", tdrv, "-o", TEXTURE_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the SfM global BA's driver (SfMGlobalBA, GlobalBundleAdjustment, RefineCameraPose: K31)
    sdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_sfm_driver.cpp")
    if os.path.exists(sdrv) and (force or not os.path.exists(SFM_DRIVER) or
                                 os.path.getmtime(SFM_DRIVER) < max(os.path.getmtime(sdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", sdrv, "-o", SFM_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the structure driver (TriangulateTracks, EstimateStructure, then GlobalBundleAdjustment: K32)
    udrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_structure_driver.cpp")
    if os.path.exists(udrv) and (force or not os.path.exists(STRUCTURE_DRIVER) or
                                 os.path.getmtime(STRUCTURE_DRIVER) < max(os.path.getmtime(udrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", udrv, "-o", STRUCTURE_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the matching driver (MatchImagePairs into TriangulateTracks: K33)
    mdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_match_driver.cpp")
    if os.path.exists(mdrv) and (force or not os.path.exists(MATCH_DRIVER) or
                                 os.path.getmtime(MATCH_DRIVER) < max(os.path.getmtime(mdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", mdrv, "-o", MATCH_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the relative-pose driver (MatchImagePairs into FilterImagePairs: K34)
    edrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_essential_driver.cpp")
    if os.path.exists(edrv) and (force or not os.path.exists(ESSENTIAL_DRIVER) or
                                 os.path.getmtime(ESSENTIAL_DRIVER) < max(os.path.getmtime(edrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", edrv, "-o", ESSENTIAL_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the retrieval driver (InitImagePairs into MatchImagePairs: K35)
    vdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_vlad_driver.cpp")
    if os.path.exists(vdrv) and (force or not os.path.exists(VLAD_DRIVER) or
                                 os.path.getmtime(VLAD_DRIVER) < max(os.path.getmtime(vdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", vdrv, "-o", VLAD_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the refinement driver (MatchImagePairs into FilterImagePairsFull: K34, K36, the scale and the pair graph)
    rdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_relpose_driver.cpp")
    if os.path.exists(rdrv) and (force or not os.path.exists(RELPOSE_DRIVER) or
                                 os.path.getmtime(RELPOSE_DRIVER) < max(os.path.getmtime(rdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", rdrv, "-o", RELPOSE_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the depth-map driver (ComputeDepthImage into FilterImagePairsFull: K37) and the stand-alone check of the K37 core (no device; its own main)
    ddrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_depthfill_driver.cpp")
    if os.path.exists(ddrv) and (force or not os.path.exists(DEPTHFILL_DRIVER) or
                                 os.path.getmtime(DEPTHFILL_DRIVER) < max(os.path.getmtime(ddrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", ddrv, "-o", DEPTHFILL_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    dchk = os.path.join(HERE, "..", "tests", "cpp", "depthfill_core_check.cpp")
    core = os.path.join(HERE, "csrc", "pvlm_depthfill_core.h")
    if os.path.exists(dchk) and (force or not os.path.exists(DEPTHFILL_CHECK) or
                                 os.path.getmtime(DEPTHFILL_CHECK) < max(os.path.getmtime(dchk), os.path.getmtime(core))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-DDEPTHFILL_CHECK_MAIN", dchk, "-o", DEPTHFILL_CHECK])
    # the stand-alone check of the dispatch order of the fused kernel on a point table (csrc/pvlm_dispatch_core.h; no device; its own main)
    ochk = os.path.join(HERE, "..", "tests", "cpp", "dispatch_order_driver.cpp")
    ocore = os.path.join(HERE, "csrc", "pvlm_dispatch_core.h")
    if os.path.exists(ochk) and (force or not os.path.exists(DISPATCH_ORDER_CHECK) or
                                 os.path.getmtime(DISPATCH_ORDER_CHECK) < max(os.path.getmtime(ochk), os.path.getmtime(ocore))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-DDISPATCH_ORDER_MAIN", ochk, "-o", DISPATCH_ORDER_CHECK])
    # the scale driver (ComputeDepthImage + FilterImagePairsFull against ComputeDepthImageResident + the resident overload: K39)
    cdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_scale_driver.cpp")
    if os.path.exists(cdrv) and (force or not os.path.exists(SCALE_DRIVER) or
                                 os.path.getmtime(SCALE_DRIVER) < max(os.path.getmtime(cdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", cdrv, "-o", SCALE_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the feature driver (ReadImages into InitImagePairs and MatchImagePairs: K41)
    xdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_sift_driver.cpp")
    if os.path.exists(xdrv) and (force or not os.path.exists(SIFT_DRIVER) or
                                 os.path.getmtime(SIFT_DRIVER) < max(os.path.getmtime(xdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", xdrv, "-o", SIFT_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    # the translation-averaging driver (EstimateGlobalTranslation, TranslationAveragingL2IRLS on the host compile or through the device: K42) and the host compile
    # of the K42 core for the tests
    gdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_transavg_driver.cpp")
    if os.path.exists(gdrv) and (force or not os.path.exists(TRANSAVG_DRIVER) or
                                 os.path.getmtime(TRANSAVG_DRIVER) < max(os.path.getmtime(gdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", gdrv, "-o", TRANSAVG_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_transavg_check()
    # the rotation-averaging driver (EstimateGlobalRotation into EstimateGlobalTranslation and the pieces of the former, on the host compile or through the device:
    # K40) and the host compile of the K40 core for the tests
    adrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_rotavg_driver.cpp")
    if os.path.exists(adrv) and (force or not os.path.exists(ROTAVG_DRIVER) or
                                 os.path.getmtime(ROTAVG_DRIVER) < max(os.path.getmtime(adrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", adrv, "-o", ROTAVG_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_rotavg_check()
    # the BATA driver (TranslationAveragingBATA by hand and EstimateGlobalTranslation with it, on the host compile or through the device: K44) and the host compile
    # of the K44 core for the tests
    bdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_bata_driver.cpp")
    if os.path.exists(bdrv) and (force or not os.path.exists(BATA_DRIVER) or
                                 os.path.getmtime(BATA_DRIVER) < max(os.path.getmtime(bdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", bdrv, "-o", BATA_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_bata_check()
    # the least-square start's driver (RotationAveragingLeastSquare by hand, EstimateGlobalRotation with method 2 and its chain into EstimateGlobalTranslation, on
    # the host compile or through the device: K45) and the host compile of the K45 core for the tests
    qdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_rotstart_driver.cpp")
    if os.path.exists(qdrv) and (force or not os.path.exists(ROTSTART_DRIVER) or
                                 os.path.getmtime(ROTSTART_DRIVER) < max(os.path.getmtime(qdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", qdrv, "-o", ROTSTART_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_rotstart_check()
    # the direction-based translation averaging's driver (TranslationAveragingL2Chordal and TranslationAveragingLUD by hand, EstimateGlobalTranslation with methods
    # 3 and 6, on the host compile or through the device: K46) and the host compile of the K46 core for the tests
    wdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_transdir_driver.cpp")
    if os.path.exists(wdrv) and (force or not os.path.exists(TRANSDIR_DRIVER) or
                                 os.path.getmtime(TRANSDIR_DRIVER) < max(os.path.getmtime(wdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", wdrv, "-o", TRANSDIR_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_transdir_check()
    # the minimax programme's driver (TranslationAveragingL1 by hand and EstimateGlobalTranslation with method 2, on the host compile or through the device: K47) and
    # the host compile of the K47 core for the tests
    ldrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_translp_driver.cpp")
    if os.path.exists(ldrv) and (force or not os.path.exists(TRANSLP_DRIVER) or
                                 os.path.getmtime(TRANSLP_DRIVER) < max(os.path.getmtime(ldrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", ldrv, "-o", TRANSLP_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_translp_check()
    # the triplet driver (FindTripletDevice, FilterByTripletDevice, EstimateGlobalRotation and TranslationAveragingL1 with device_triplets, on the host compile or
    # through the device: K48) and the host compile of the K48 core for the tests
    pdrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_triplet_driver.cpp")
    if os.path.exists(pdrv) and (force or not os.path.exists(TRIPLET_DRIVER) or
                                 os.path.getmtime(TRIPLET_DRIVER) < max(os.path.getmtime(pdrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", pdrv, "-o", TRIPLET_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_triplet_check()
    # the neighbour-selection driver (SelectNeighborSFM and SelectNeighborViews on the literal host loop or through the device: K49) and the host compile of the K49
    # core for the tests
    ndrv = os.path.join(HERE, "..", "tests", "cpp", "pvlm_neighbor_driver.cpp")
    if os.path.exists(ndrv) and (force or not os.path.exists(NEIGHBOR_DRIVER) or
                                 os.path.getmtime(NEIGHBOR_DRIVER) < max(os.path.getmtime(ndrv), os.path.getmtime(HOST_LIB))):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", ndrv, "-o", NEIGHBOR_DRIVER, "-L" + HERE, "-lpvlm_host", "-lpvlm",
                               "-Wl,-rpath," + HERE])
    build_neighbor_sfm_check()
    return HOST_LIB


def _include_closure(src):
    """src and every file it reaches through #include "..." lines, transitively."""
    seen, todo = set(), [os.path.normpath(src)]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(f):
            continue
        seen.add(f)
        todo += [os.path.normpath(os.path.join(os.path.dirname(f), m)) for m in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), re.M)]
    return sorted(seen)


def build_core_check(kind, main=False, sanitize=False):
    """The host compile of a pair-graph stage's core (kind "transavg": K42, "rotavg": K40, "bata": K44, "rotstart": K45, "transdir": K46, "translp": K47, "triplet": K48, "neighbor_sfm": K49; csrc/pvlm_<kind>_core.h behind tests/cpp/<kind>_core_check.cpp; no device,
    -ffp-contract=off as the device build of pvlm_<kind>.hip): build/lib<kind>_check.so for the tests, or with main=True the stand-alone program of the same file
    (sanitize: the host sanitizers).  Rebuilt when the source or any header it includes, directly or not, is newer."""
    chk = os.path.join(HERE, "..", "tests", "cpp", kind + "_core_check.cpp")
    out = os.path.join(HERE, "build", kind + "_check_main" if main else "lib" + kind + "_check.so")
    if not os.path.exists(chk):
        return None
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if main or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in _include_closure(chk)):
        mode = ["-O1", "-g", "-D%s_CHECK_MAIN" % kind.upper()] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []) if main else ["-O2", "-fPIC", "-shared"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off"] + mode + [chk, "-o", out])
    return out


def build_transavg_check(main=False, sanitize=False):
    return build_core_check("transavg", main, sanitize)


def build_rotavg_check(main=False, sanitize=False):
    return build_core_check("rotavg", main, sanitize)


def build_bata_check(main=False, sanitize=False):
    return build_core_check("bata", main, sanitize)


def build_rotstart_check(main=False, sanitize=False):
    return build_core_check("rotstart", main, sanitize)


def build_transdir_check(main=False, sanitize=False):
    return build_core_check("transdir", main, sanitize)


def build_translp_check(main=False, sanitize=False):
    return build_core_check("translp", main, sanitize)


def build_triplet_check(main=False, sanitize=False):
    return build_core_check("triplet", main, sanitize)


def build_neighbor_sfm_check(main=False, sanitize=False):
    return build_core_check("neighbor_sfm", main, sanitize)


if __name__ == "__main__":
    if "--variant" in sys.argv:
        k = sys.argv.index("--variant")
        print(build_variant(sys.argv[k + 1], [a for a in sys.argv[k + 2:] if a.startswith("-D")]))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
        print(build_host(force="--force" in sys.argv))
