"""The chunked resolution of the drawSpheres / multiSpheres walk (csrc/sphere_walk.h), checked on the CPU."""
import os
import shutil
import subprocess


def test_chunked_walk_equals_the_serial_walk(mvs, tmp_path):
    """tests/c_abi/sphere_walk_main.cpp: csrc/sphere_walk.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a child
    process, nothing preloaded) against a serial walk over java.util.Random written in the program.  Large-sphere radii 0, 1 and 16, both
    acceptance rules, bounds 10 and 20, seeds 1..8, chunks of 512, 513 and the library's own: the same accepted voxels (ordinal, raw
    nextInt, value), the same final state and step count; composing runs of chunks equals walking them.  Crafted states that make voxel
    m retry nextInt once, m = 0, 1 and the three values around chunk / 3 (found within low < 2^17 or the program fails), as whole walks
    and as walks that end with voxel m.  One entry offset, or an event list of one entry, raise the flag instead of a wrong answer."""
    exe = str(tmp_path / "sphere_walk_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "sphere_walk_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sphere walk ok: 410 cases" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
