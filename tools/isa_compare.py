"""Do two sets of sources compile to the same kernels?

    python tools/isa_compare.py --old OLD.hip [...] --new NEW.hip [...] [--asm-dir DIR [--reuse]]

Compiles every file to gfx950 assembly with the product's flags (device only, nothing is linked or run: works without a GPU), collects the
kernels of each side (the `.amdhsa_kernel` symbols) and compares, per kernel, the instruction lines between the symbol's label and its
`.Lfunc_end` -- without assembler comments (everything from `;`) and blank lines, and with the function number taken out of local labels
(`.LBB<n>_<m>` -> `.LBB_<m>`: it counts the functions of the translation unit) -- and the figures of the compiler's resource remarks
(registers, spills, scratch, occupancy, LDS).  One line per kernel that differs or exists on one side only; exit status 1 on any difference.
What a refactor that only moves kernels between translation units has to show.  --asm-dir keeps the assembly and the remarks (as
old_<file>.s / new_<file>.s); with --reuse a file already there is taken as it is instead of compiled again.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I/opt/rocm/include",
         "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]
FIGURES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
           "LDS Size [bytes/block]")


def compile_one(src, out, reuse):
    """-> (assembly text, remarks text) of one source file"""
    if not (reuse and os.path.exists(out) and os.path.exists(out + ".remarks")):
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, src], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"{src}:\n{r.stderr}")
        with open(out + ".remarks", "w") as fh:
            fh.write(r.stderr)
    return open(out).read(), open(out + ".remarks").read()


def kernels_of(asm, remarks):
    """-> {kernel symbol: (instruction lines, {figure: value})}"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    body, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(\S+):", line)
        if cur is None:
            if m and m.group(1) in names:
                cur = m.group(1)
                body[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        if line:
            body[cur].append(line)
    figures, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, value = m.group(1).partition(": ")
        if key == "Function Name":
            cur = value.strip()
            figures[cur] = {}
        elif cur is not None and key.strip() in FIGURES:
            figures[cur][key.strip()] = value.strip()
    missing = [k for k in names if k not in body or k not in figures]
    if missing:
        raise SystemExit(f"no body or no resource remarks for {missing[:3]} ...")
    return {k: (body[k], figures[k]) for k in names}


def side(tag, texts):
    kernels = {}
    for asm, remarks in texts:
        for k, v in kernels_of(asm, remarks).items():
            if k in kernels:
                raise SystemExit(f"{tag}: kernel {k} is defined twice")
            kernels[k] = v
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--asm-dir")
    ap.add_argument("--reuse", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm_dir = a.asm_dir or tmp
        os.makedirs(asm_dir, exist_ok=True)
        jobs = [(s, os.path.join(asm_dir, f"{tag}_{os.path.basename(s)}.s")) for tag, srcs in (("old", a.old), ("new", a.new)) for s in srcs]
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:           # (the files of both sides side by side)
            texts = list(ex.map(lambda so: compile_one(so[0], so[1], a.reuse), jobs))
        old, new = side("old", texts[:len(a.old)]), side("new", texts[len(a.old):])
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in new or k not in old:
            print(f"only in {'old' if k in old else 'new'}: {k}")
            bad += 1
            continue
        what = []
        if old[k][0] != new[k][0]:
            first = next((i for i, (x, y) in enumerate(zip(old[k][0], new[k][0])) if x != y), min(len(old[k][0]), len(new[k][0])))
            what.append(f"code ({len(old[k][0])} -> {len(new[k][0])} lines, first difference at line {first})")
        what += [f"{f} {old[k][1].get(f)} -> {new[k][1].get(f)}" for f in FIGURES if old[k][1].get(f) != new[k][1].get(f)]
        if what:
            print(f"differs: {k}: " + ", ".join(what))
            bad += 1
    print(f"{len(old)} kernels old, {len(new)} kernels new, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
