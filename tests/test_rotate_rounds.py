"""The round schedule both roles of the role-split fused rotate kernel iterate (csrc/rotate_rounds.h), checked on the CPU."""
import os
import shutil
import subprocess


def test_round_schedule_of_walkers_and_transformers(mvs, tmp_path):
    """tests/c_abi/rotate_rounds_main.cpp: csrc/rotate_rounds.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a
    child process, nothing preloaded).  steps 1..40, 63, 64, 65, 511, 512, chunks of 128 and 512 rows, 2 and 4 transformers, class
    tables all 0 / 1 / 2, alternating, random: the roles see the same rounds in the same buffers, every row is transformed or
    zero-stored exactly once, no buffer is refilled while its round is read.  No mismatch, no sanitizer report."""
    exe = str(tmp_path / "rotate_rounds_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "rotate_rounds_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rotate rounds ok: 900 cases" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]


def test_row_walk_arithmetic_equals_the_oracle(mvs, tmp_path):
    """tests/c_abi/row_geometry_main.cpp: csrc/rotate_dev.h -- the one statement of the rotate kernels' row geometry, blend and
    attenuation step -- compiled by the host compiler with -O2 -ffp-contract=off and linked with oracle/mvsim_oracle.c (no HIP, no
    libmvsim.so; a child process, nothing preloaded).  Nx 5, Ny 37, Nz 29; 0, 15, 33, -52, 90, 180 degrees about x: rot_value and
    row_geometry + load_taps_masked + blend4 both equal the oracle's rotateAroundAxis bit for bit, attenuate_step down every column
    equals attenuate3d bit for bit (delta 0.01, 0.4); at 33 degrees rows of every kind (none, all taps inside, partial) occur."""
    here = os.path.dirname(os.path.abspath(__file__))
    orc_dir = os.path.join(os.path.dirname(here), "oracle")
    obj, exe = str(tmp_path / "mvsim_oracle.o"), str(tmp_path / "row_geometry_main")
    fp = ["-O2", "-ffp-contract=off", "-fno-fast-math"]
    cmds = [[shutil.which("gcc") or "gcc", "-std=c11", *fp, "-c", os.path.join(orc_dir, "mvsim_oracle.c"), "-o", obj],
            [shutil.which("g++") or "g++", "-std=c++17", *fp, "-Wall", "-Wextra", "-Werror", "-I" + orc_dir,
             "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"), os.path.join(here, "c_abi", "row_geometry_main.cpp"), obj,
             "-lm", "-o", exe]]
    for cmd in cmds:
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "row geometry ok: 6 rotations" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
