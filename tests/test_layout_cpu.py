"""The buffer layouts of the LiDAR feature front end (panovlm_amd/csrc/pvlm_layout.h: ring results, line-growth input and output, undistort staging) through
tests/cpp/layout_check.cpp: a stand-alone program built with AddressSanitizer and UBSan that mallocs exactly the size a layout asks for, writes every region end
to end at its full capacity and asserts the regions disjoint and aligned — over point counts around the 64-byte steps, odd and even numbers of scans (the odd
ones are where a size formula and an offset formula written apart disagreed by four bytes), with and without picks.  A child process: nothing is loaded here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_region_fits_the_size_its_layout_asks_for(tmp_path):
    exe = str(tmp_path / "layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "layout_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.split("\n")
    assert "ring: 72 layouts" in lines and "line growth: 30 layouts" in lines and "undistort: 8 layouts" in lines and "ok" in lines
