#!/usr/bin/env python3
"""Says, kernel by kernel, whether a .hip file compiles to the same gfx950 code in the working tree as at a git revision: the check of a refactor
that must not change the device code.  Both trees are compiled device-only to assembly with the flags of panovlm_amd/build.py (PVLM_DEFINES
honoured); what differs between any two builds (.file / .loc / .ident, comment lines, the __hip_cuid_* symbol) is dropped before comparing.
A kernel's text runs from its label to the end of its .amdhsa_kernel block (registers, LDS, scratch); "(outside the kernels)" is the rest: data
and the metadata with the kernarg layouts.  Needs no GPU.  Exit status 1 when anything differs.
usage: python tools/isa_same.py FILE.hip [REV]   (REV defaults to HEAD)"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from panovlm_amd.build import ARCH, NO_CONTRACT, _hipcc  # noqa: E402


def assembly(tree, rel):
    base = os.path.basename(rel)
    flags = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-w"] + os.environ.get("PVLM_DEFINES", "").split()
    flags += ["-ffp-contract=off"] if base in NO_CONTRACT else []
    flags += ["-fno-slp-vectorize"] if base == "pvlm_assoc.hip" else []
    return subprocess.Popen([_hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(tree, rel), "-o", "-"], stdout=subprocess.PIPE, text=True)


def kernels(text):
    """{kernel: its lines} and the lines outside every kernel, without what differs from build to build"""
    lines = [l for l in text.split("\n") if l.strip() and not re.match(r"\s*(;|\.file\s|\.loc\s|\.ident\s)", l) and "__hip_cuid_" not in l]
    # local labels carry the function's number in the module (.LBB<function>_<block>), which moves when kernels are added or removed in front of it
    lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines]
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, rest, cur = {}, [], None
    for l in lines:
        label = re.match(r"(\S+):", l)
        if cur is None and label and label.group(1) in names:
            cur = label.group(1)
            out[cur] = []
        (rest if cur is None else out[cur]).append(l)
        if cur is not None and l.strip() == ".end_amdhsa_kernel":
            cur = None
    return out, rest


def main():
    rel = os.path.relpath(os.path.abspath(sys.argv[1]), ROOT)
    rev = sys.argv[2] if len(sys.argv) > 2 else "HEAD"
    with tempfile.TemporaryDirectory() as d:
        subprocess.run("git -C '%s' archive '%s' | tar -x -C '%s'" % (ROOT, rev, d), shell=True, check=True)
        jobs = [assembly(ROOT, rel), assembly(d, rel)]
        texts = [j.communicate()[0] for j in jobs]
    if any(j.returncode for j in jobs):
        sys.exit("hipcc failed on " + rel)
    (new, new_rest), (old, old_rest) = kernels(texts[0]), kernels(texts[1])
    count = lambda body: sum(1 for l in body if re.match(r"\s+[a-z]\w*(\s|$)", l))   # instructions: neither labels nor directives
    differs = 0
    for name in sorted(set(new) | set(old)):
        same = new.get(name) == old.get(name)
        differs += not same
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()[:120]
        print("%-120s %s" % (short, "identical" if same else "differs (%d vs %d instructions)" % (count(new.get(name, [])), count(old.get(name, [])))))
    print("%-120s %s" % ("(outside the kernels)", "identical" if new_rest == old_rest else "differs"))
    print("%s against %s: %d kernels, %d identical, %d differ" % (rel, rev, len(set(new) | set(old)), len(set(new) | set(old)) - differs, differs))
    sys.exit(1 if differs or new_rest != old_rest else 0)


if __name__ == "__main__":
    main()
