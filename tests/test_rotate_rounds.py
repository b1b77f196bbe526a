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
