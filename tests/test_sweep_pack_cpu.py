"""The packed sweep grid's set-up logic (gibbssampler_amd/csrc/gs_sweep_pack.h)
on the CPU: tests/sweep_pack_check.cpp, a stand-alone program built from the
header with the host compiler under AddressSanitizer and UBSan, walks the grid
as the kernel does and checks that every (l, m) of the triangle lies in exactly
one segment of one workgroup, that segments stay inside a chunk and that no
thread index or LDS slot is out of range (the program's header lists it all)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LS = [0, 1, 63, 64, 70, 96, 127, 128, 130, 300, 320, 520, 576, 1024]
# what the shapes of tests/test_gpu_sweep_pack.py are there for: the number of
# absorbed one-entry groups, of packed workgroups that hold row m = 0, and of
# packed workgroups of a partial tile (lanes l < 0)
GPU_SHAPES = {70: (0, 0, 0), 96: (2, 1, 1), 127: (0, 1, 0), 128: (2, 0, 0), 130: (0, 0, 0), 300: (0, 1, 3),
              320: (5, 0, 0), 520: (0, 1, 0), 576: (9, 1, 0)}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sweep_pack") / "sweep_pack_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "gibbssampler_amd", "csrc"), "-o", exe,
                    os.path.join(HERE, "sweep_pack_check.cpp")], check=True)
    r = subprocess.run([exe] + [str(L) for L in LS], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    out = {}
    for ln in r.stdout.splitlines():
        L, tm, nwg, npacked, nabsorb, plain, issued, m0, partial = (int(x) for x in ln.split())
        out[L] = dict(tm=tm, nwg=nwg, npacked=npacked, nabsorb=nabsorb, plain=plain, issued=issued, m0=m0,
                      partial=partial)
    return out


def test_every_shape_checks(lines):
    assert sorted(lines) == LS
    for L, v in lines.items():
        assert v["tm"] == (16 if L > 512 else 4 if L > 256 else 8)
        assert v["issued"] <= v["plain"]


def test_gpu_test_shapes_reach_every_path(lines):
    """The shapes the GPU on/off test runs pack at least one workgroup each, and
    the ones chosen for the absorbed single entry, the row m = 0 taken before
    the loop and the lanes l < 0 do hold them (an absorbing shape needs l_hi a
    multiple of 4 chunks: L a multiple of 64 / 32 / 16 at 16 / 8 / 4 rows)."""
    for L, (nabsorb, m0, partial) in GPU_SHAPES.items():
        v = lines[L]
        assert v["npacked"] > 0, L
        assert (v["nabsorb"], v["m0"], v["partial"]) == (nabsorb, m0, partial), L
    assert sum(1 for a, _, _ in GPU_SHAPES.values() if a) >= 4


def test_flagship_counts(lines):
    """L 1024, 16 rows per chunk: the plain grid's 153 workgroups and 8 721
    wave-rows per chain (profiles/r06_sweep_issue_model.json: x 32 chains).  A
    wave-row holds 64 lane slots and the triangle 525 825 entries, so no grid
    issues fewer than 8 216 = 8 721 - 505 wave-rows; segments are not split, so
    a diagonal workgroup's 104 full 16-row segments alone hold two waves for 16
    rows each.  With one segment per thread the 24 longest short ones (15 .. 10
    rows) fill those two waves and the third runs 9 rows, 41 against 64 + 1; the
    tile whose diagonal workgroup holds row m = 0 takes that one-slot row before
    the loop in each of its three waves (44).  The 120 full workgroups and the
    tile l = 0 stay: 120 x 64 + 1 + 15 x 41 + 44 = 8 340."""
    v = lines[1024]
    assert v["plain"] == 8721 and v["nwg"] + v["nabsorb"] == 153
    assert v["nabsorb"] == 16 and v["npacked"] == 16
    assert 8216 <= v["issued"] == 120 * 64 + 1 + 15 * 41 + 44
