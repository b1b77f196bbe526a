"""The per-voxel arithmetic of the Poisson sampler (csrc/poisson_recipe.h), held to the oracle on the CPU."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def recipe_exe(mvs, tmp_path_factory):
    """tests/c_abi/poisson_recipe_main.cpp: csrc/poisson_recipe.h compiled by the host compiler with -O2 -ffp-contract=off under ASan +
    UBSan (no HIP include, no libmvsim.so) and linked with oracle/mvsim_oracle.c into a program of its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    orc_dir = os.path.join(os.path.dirname(here), "oracle")
    tmp = tmp_path_factory.mktemp("poisson_recipe")
    obj, exe = str(tmp / "mvsim_oracle.o"), str(tmp / "poisson_recipe_main")
    fp = ["-O2", "-ffp-contract=off", "-fno-fast-math"]
    cmds = [[shutil.which("gcc") or "gcc", "-std=c11", *fp, "-c", os.path.join(orc_dir, "mvsim_oracle.c"), "-o", obj],
            [shutil.which("g++") or "g++", "-std=c++17", *fp, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
             "-Werror", "-I" + orc_dir, "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
             os.path.join(here, "c_abi", "poisson_recipe_main.cpp"), obj, "-lm", "-o", exe]]
    for cmd in cmds:
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stdout + b.stderr
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)      # a child process, nothing preloaded
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r


def test_poisson_voxel_equals_the_oracle(recipe_exe):
    """3 000 000 tuples: lambda log-uniform over [1e-3, 1e15] through float plus exactly 10, the float below 10, 0, a negative value and
    NaN; three keys (low word only, both words, all ones); streams 0, 1, 2^31 - 1, 2^32 - 1; 200 000 consecutive counters from each of
    0, 2^32 - 100, 2^33 - 7, 2^63 - 50, 2^64 - 300.  poisson_voxel equals orc_poisson_counter on every one, poisson_counter4 over every
    aligned group of four gives the same counts, and the fp32 screen answered on more than a quarter of the exact tests it was shown --
    never differently from the exact test.  No mismatch, no sanitizer report."""
    r = _run(recipe_exe)
    assert r.returncode == 0 and "poisson recipe ok: 3000000 tuples" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "mismatches: poisson_voxel 0, poisson_counter4 0, without the screen 0" in r.stderr, r.stderr[-4000:]


def test_counts_do_not_depend_on_the_screen(recipe_exe):
    """The program's `noscreen` mode: the same tuples through the recipe's pieces without ptrs_screen (every attempt the squeeze leaves
    open goes to ptrs_exact) equal the oracle too."""
    r = _run(recipe_exe, "noscreen")
    assert r.returncode == 0 and "poisson recipe ok (screen-less walk): 3000000 tuples" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "without the screen 0" in r.stderr, r.stderr[-4000:]
