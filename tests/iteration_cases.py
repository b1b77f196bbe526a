"""Deterministic cases of the main-loop iteration sweep (tests/test_iteration_sweep.py): mvsim_simulate_iteration_dev, the device-resident
body of `main`'s view loop (csrc/api_view.cpp) -- the view, makeIsotropic, and the rotate-backs of the isotropic view, of the cached
weight image and of the PSF -- over every axis and angle class, both kernels of launch_rotate in all three rotate-backs, every subset of
the optional outputs, and a script of iterations through ONE long-lived context whose inputs change from view to view.

Pure Python and numpy: importable without a GPU.  The CPU tests check the table's coverage and the sensitivity of the inputs from the same
list the GPU tests run.  Shapes are numpy (nz, ny, nx) here; the library takes (nx, ny, nz)."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

SEED = 464232194
OUTPUTS = ("iso", "view", "view_weights", "view_psf")
FUSED_MIN_HALF = 72                 # rot_fftx_len_ok: the fused rotate kernel exists for padded x half lengths 72 .. 576

# the targets of part 1; each is named by at least one case whose own values land on it (landing)
TARGETS = (
    "axis0", "axis1", "axis2", "back=-degrees", "psf-even-extent", "psf-non-cubic", "sampled", "noise-free",
    "back0", "back90", "back-90", "back180",
    "nx%4==0", "nx%4!=0", "nx20", "nx64", "nx18", "nx70",
    "misaligned-outputs", "misaligned-rotate-out-only",
    "kx%4==0", "kx%4!=0",
    "ny-even", "ny-odd", "niso-even", "niso-odd", "niso!=nz",
    "inc1", "inc2", "inc3", "inc4", "(nz-1)%inc==0", "(nz-1)%inc!=0", "nz12", "nz13", "nz17",
    "conv1", "conv2",
    "flagged-0deg-roles", "flagged-0deg-1", "flagged-3deg-roles", "flagged-3deg-1",
)


@dataclass
class Case:
    name: str
    shape: tuple               # (nz, ny, nx)
    kshape: tuple              # (kz, ky, kx)
    axis: int
    degrees: int
    back: int
    targets: tuple             # what this case is in the sweep for
    inc: int = 1
    snr: float = -1.0          # < 0: noise-free (acq against the fp64 oracle); >= 0: sampled (acq against mvsim_simulate_view_dev)
    conv_method: int = 1
    opts: dict = field(default_factory=dict)
    offsets: dict = field(default_factory=dict)      # output name -> floats past a 16-byte boundary
    specimen: str = "phantom"  # "phantom": sphere phantom + specks; "slab": random values in a few middle planes (empty planes around them)

    @property
    def id(self) -> str:
        return self.name

    @property
    def dim(self):
        return self.shape[::-1]

    @property
    def nzo(self) -> int:
        return (self.shape[0] - 1) // self.inc + 1

    @property
    def niso(self) -> int:
        return (self.nzo - 1) * self.inc + 1

    @property
    def seed(self) -> int:
        return SEED + zlib.crc32(self.name.encode()) % 1000

    @property
    def stream(self) -> int:
        return 1 + zlib.crc32(self.name.encode()) % 5

    def out_shapes(self) -> dict:
        nz, ny, nx = self.shape
        return {"acq": (self.nzo, ny, nx), "iso": (self.niso, ny, nx), "view": (self.niso, ny, nx), "view_weights": (nz, ny, nx),
                "view_psf": tuple(self.kshape)}


A_SHAPE, A_PSF = (13, 22, 20), (4, 5, 3)
B_SHAPE, B_PSF = (11, 13, 9), (3, 6, 5)
F_SHAPE, F_PSF = (24, 128, 128), (5, 5, 17)          # the smallest the fused rotate kernel takes (tests/test_skip_tail.py)


def cases():
    """Every case of part 1, in a fixed order: the smallest shapes at which each thing can still go wrong."""
    out = []
    # ---- every axis, back = -degrees, non-cubic PSFs with one even extent; the larger shape sampled, the smaller noise-free
    for axis, deg in ((0, 33), (1, -52), (2, 123)):
        out.append(Case(f"axis{axis}-A", A_SHAPE, A_PSF, axis, deg, -deg, (f"axis{axis}", "back=-degrees", "psf-even-extent", "psf-non-cubic",
                                                                           "sampled", "nx20"), inc=2, snr=25.0))
        out.append(Case(f"axis{axis}-B", B_SHAPE, B_PSF, axis, -deg, deg, (f"axis{axis}", "back=-degrees", "psf-even-extent", "psf-non-cubic",
                                                                           "noise-free"), inc=3))
    # ---- back angles whose taps lie exactly on the grid, about x; ny odd
    for back in (0, 90, -90, 180):
        out.append(Case(f"back{back}", (12, 21, 20), (3, 5, 4), 0, 20, back, (f"back{back}", "ny-odd", "kx%4==0", "nz12"), inc=1))
    # ---- both kernels of launch_rotate by nx % 4, in the iso / weights rotations (the PSF's own by kx % 4)
    out.append(Case("nx64", (7, 66, 64), (3, 3, 8), 0, 40, -40, ("nx64", "nx%4==0", "kx%4==0", "ny-even"), inc=2))
    out.append(Case("nx70", (7, 72, 70), (3, 3, 5), 0, 40, -40, ("nx70", "nx%4!=0", "kx%4!=0"), inc=2))
    out.append(Case("nx18", (9, 20, 18), (3, 5, 4), 0, -25, 25, ("nx18", "nx%4!=0", "kx%4==0"), inc=1, snr=25.0))
    out.append(Case("nx20-kx3", (9, 20, 20), (3, 5, 3), 0, -25, 25, ("nx20", "nx%4==0", "kx%4!=0"), inc=1))
    # ---- the same by alignment: every output 4 bytes past a 16-byte boundary; then the rotate-backs' outputs alone (aligned sources)
    off = {k: 1 for k in ("acq",) + OUTPUTS}
    out.append(Case("misaligned", (9, 20, 20), (3, 5, 4), 0, 33, -33, ("misaligned-outputs",), inc=2, offsets=off))
    out.append(Case("misaligned-sampled", (9, 20, 20), (3, 5, 4), 0, 33, -33, ("misaligned-outputs", "sampled"), inc=2, snr=25.0, offsets=off))
    out.append(Case("misaligned-backs", (9, 20, 20), (3, 5, 4), 0, 33, -33, ("misaligned-rotate-out-only",), inc=2,
                    offsets={"view": 1, "view_weights": 1, "view_psf": 1}))
    # ---- inc with (nz - 1) % inc zero and non-zero; centre parity of the isotropic volume
    for inc, nz in ((1, 13), (2, 13), (2, 12), (3, 13), (3, 17), (4, 13), (4, 12), (3, 12)):
        c = Case(f"inc{inc}-nz{nz}", (nz, 22, 20), A_PSF, 0, -52, 52, (), inc=inc)
        t = [f"inc{inc}", f"nz{nz}", "(nz-1)%inc==0" if (nz - 1) % inc == 0 else "(nz-1)%inc!=0", "niso-even" if c.niso % 2 == 0 else "niso-odd"]
        if c.niso != nz:
            t.append("niso!=nz")
        c.targets = tuple(t)
        out.append(c)
    # ---- the stencil: no spectrum, never cached
    out.append(Case("stencil", A_SHAPE, A_PSF, 0, 33, -33, ("conv2",), inc=2, conv_method=2))
    out.append(Case("stencil-sampled", A_SHAPE, A_PSF, 1, 33, -33, ("conv2", "sampled"), inc=2, snr=25.0, conv_method=2))
    out.append(Case("fft", A_SHAPE, A_PSF, 0, 33, -33, ("conv1",), inc=2, conv_method=1))
    # ---- the flagged fused kernel: an iteration whose acq comes from the sparse tail
    for deg, inc in ((0, 1), (3, 3)):
        for mode in ("roles", 1):
            out.append(Case(f"flagged-{deg}deg-{mode}", F_SHAPE, F_PSF, 0, deg, -deg, (f"flagged-{deg}deg-{mode}", "sampled"), inc=inc, snr=25.0,
                            opts={"fused_fftx": mode}, specimen="slab"))
    return out


def landing(c: Case) -> set:
    """Every target the case's own values land on -- computed from the values, not from what the case claims."""
    nz, ny, nx = c.shape
    kz, ky, kx = c.kshape
    out = {f"axis{c.axis}", f"inc{c.inc}", f"conv{c.conv_method}", "sampled" if c.snr >= 0 else "noise-free"}
    if c.back == -c.degrees and c.degrees in (33, -33, -52, 52, 123, -123):
        out.add("back=-degrees")
    if any(k % 2 == 0 for k in c.kshape):
        out.add("psf-even-extent")
    if len(set(c.kshape)) > 1:
        out.add("psf-non-cubic")
    if c.axis == 0 and c.back in (0, 90, -90, 180):
        out.add(f"back{c.back}")
    out.add("nx%4==0" if nx % 4 == 0 else "nx%4!=0")
    if nx in (18, 20, 64, 70):
        out.add(f"nx{nx}")
    out.add("kx%4==0" if kx % 4 == 0 else "kx%4!=0")
    if c.offsets and all(c.offsets.get(k, 0) % 4 != 0 for k in ("acq",) + OUTPUTS):
        out.add("misaligned-outputs")
    if c.offsets and all(c.offsets.get(k, 0) % 4 != 0 for k in ("view", "view_weights", "view_psf")) and \
            all(c.offsets.get(k, 0) % 4 == 0 for k in ("acq", "iso")) and nx % 4 == 0:
        out.add("misaligned-rotate-out-only")
    out.add("ny-even" if ny % 2 == 0 else "ny-odd")
    out.add("niso-even" if c.niso % 2 == 0 else "niso-odd")
    if c.niso != nz:
        assert (nz - 1) % c.inc != 0
        out.add("niso!=nz")
    out.add("(nz-1)%inc==0" if (nz - 1) % c.inc == 0 else "(nz-1)%inc!=0")
    if nz in (12, 13, 17):
        out.add(f"nz{nz}")
    if "fused_fftx" in c.opts and c.opts["fused_fftx"] in ("roles", 1) and c.axis == 0 and 64 <= nx <= ny and c.specimen == "slab" and c.snr >= 0 \
            and c.conv_method == 1:
        out.add(f"flagged-{c.degrees}deg-{c.opts['fused_fftx']}")
    return out


# ------------------------------------------------------------------------------------------------ inputs
def phantom(synth, shape, seed=91):
    """The sphere phantom plus seeded random specks (tests/test_rotate_forms.py): no mirror symmetry."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.02).astype(np.float32))


def slab(shape, planes=None, seed=77, scale=1.0, offset=0.25):
    """Random values confined to `planes` (default: four middle ones) and to the middle quarter of y: empty planes around a specimen that a
    small angle keeps thin (tests/test_skip_tail.py)."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype=np.float32)
    planes = range(nz // 2 - 2, nz // 2 + 2) if planes is None else planes
    y0, y1 = ny // 2 - max(1, ny // 8), ny // 2 + max(1, ny // 8)
    for z in planes:
        v[z, y0:y1, :] = (rng.random((y1 - y0, nx), dtype=np.float32) + np.float32(offset)) * np.float32(scale)
    return v


def random_psf(kshape, seed):
    """rng.random + 0.05: no symmetry, no zero tap."""
    return np.random.default_rng(seed).random(kshape, dtype=np.float32) + np.float32(0.05)


def case_inputs(synth, c: Case):
    """(ground truth, this view's raw PSF, the raw PSF of the view before it)."""
    s = zlib.crc32(c.name.encode())
    gt = slab(c.shape, seed=s % 1000) if c.specimen == "slab" else phantom(synth, c.shape, seed=91 + s % 100)
    return gt, random_psf(c.kshape, s), random_psf(c.kshape, s + 1)


# ------------------------------------------------------------------------------------------------ part 2: the script
A_ANGLES = (33, -52, 123, -90)


@dataclass(frozen=True)
class Step:
    """One iteration of the script.  Steps that compare equal are the same iteration: one fresh-context reference, one set of output buffers
    in the synchronised modes (so that option graph sees the same key again)."""
    shape: tuple
    gt: str                    # name of the ground truth (volumes)
    psf: int                   # seed of the PSF
    kshape: tuple
    degrees: int
    back: int
    wants: tuple               # subset of OUTPUTS
    inc: int = 1
    snr: float = 25.0
    seed: int = SEED
    stream: int = 0
    delta: float = float(np.float32(0.01))
    axis: int = 0

    @property
    def dim(self):
        return self.shape[::-1]

    @property
    def nzo(self) -> int:
        return (self.shape[0] - 1) // self.inc + 1

    @property
    def niso(self) -> int:
        return (self.nzo - 1) * self.inc + 1

    def out_shapes(self) -> dict:
        nz, ny, nx = self.shape
        full = {"acq": (self.nzo, ny, nx), "iso": (self.niso, ny, nx), "view": (self.niso, ny, nx), "view_weights": (nz, ny, nx),
                "view_psf": tuple(self.kshape)}
        return {k: full[k] for k in ("acq",) + self.wants}


NO_PSF = ("iso", "view", "view_weights")
C_SHAPE, C_PSF = (9, 26, 24), (3, 4, 5)              # the "B" of the size change A -> B -> A: other extents, fewer voxels than A
F_SPARSE_PLANES = 16                                 # the sixteen sparse volumes of the flag cycle hold 1 .. 16 planes
RELEASE = "release_caches"                           # a script entry that is no iteration


def f_planes(k: int):
    """k planes of the flagged shape, spread from plane 1 + k % 3 on (never the same set twice)."""
    nz = F_SHAPE[0]
    first = 1 + k % 3
    return tuple(range(first, first + k)) if first + k <= nz else tuple(range(nz - k, nz))


def volumes(synth) -> dict:
    """Every ground truth of the script by name.  The flagged shape's volumes are built for 0 degrees: a plane is empty behind the
    attenuation iff the specimen leaves it empty."""
    rng = np.random.default_rng(79)
    v = {"A": phantom(synth, A_SHAPE, 92), "C": phantom(synth, C_SHAPE, 93),
         "f-sparse-a": slab(F_SHAPE, (10, 11, 12, 13), 101), "f-sparse-b": slab(F_SHAPE, (3, 4, 5, 18, 19), 102),
         "f-dense": rng.random(F_SHAPE, dtype=np.float32) + np.float32(0.01),
         "f-loud": (rng.random(F_SHAPE, dtype=np.float32) + np.float32(0.5)) * np.float32(1e6),
         "f-zero": np.zeros(F_SHAPE, dtype=np.float32), "f-nan": np.full(F_SHAPE, np.nan, dtype=np.float32)}
    for k in range(1, F_SPARSE_PLANES + 1):
        v[f"f-sparse-{k}"] = slab(F_SHAPE, f_planes(k), 110 + k)
    return v


def empty_planes(name: str):
    """Empty planes of a flagged-shape volume at 0 degrees (None: not a flagged-shape volume)."""
    nz = F_SHAPE[0]
    if name == "f-sparse-a":
        return nz - 4
    if name == "f-sparse-b":
        return nz - 5
    if name in ("f-dense", "f-loud", "f-nan"):
        return 0
    if name == "f-zero":
        return nz
    if name.startswith("f-sparse-"):
        return nz - int(name.rsplit("-", 1)[1])
    return None


def script():
    """The script of part 2, in order.  The flagged shape first: it sizes every workspace, so that nothing a later, smaller view needs makes
    a workspace grow under captured graphs (twiddles and plans of a new geometry still may)."""
    out = []

    # ---- the ground truth rewritten in place at the flagged shape, across the sixteen-view flag cycle.  One key throughout (delta = 1e-9 for
    # the volume of values around 1e6): under option graph the second view is captured and every later one replays it on changed contents
    def f(gt, snr=25.0):
        return Step(F_SHAPE, gt, 500, F_PSF, 0, -3, NO_PSF, inc=1, snr=snr, stream=3, delta=1e-9)
    out += [f("f-sparse-a"), f("f-sparse-b"), f("f-dense")]
    out += [f(f"f-sparse-{k}") for k in range(1, 15)]
    out += [f("f-nan", snr=-1.0)]                       # the fifteenth view behind the dense one; every workspace it touches is NaN after it
    out += [f("f-sparse-15"), f("f-sparse-16")]         # the sixteenth carries flags again: a sparse tail right behind the NaN volume
    out += [f("f-loud"), f("f-zero"), f("f-sparse-a")]
    # ---- the `main` pattern: V angles, back = -angle, per-view PSFs, three rounds (eager, captured, replayed under option graph); views 0
    # and 2 ask for view_psf (their PSF goes round the cache), views 1 and 3 do not (a miss in round one, hits after)
    for _ in range(3):
        for v, a in enumerate(A_ANGLES):
            out.append(Step(A_SHAPE, "A", 600 + v, A_PSF, a, -a, OUTPUTS if v % 2 == 0 else NO_PSF, inc=2, snr=25.0 if v != 1 else -1.0,
                            seed=SEED + v, stream=v))
    # ---- the decisive pair: PSF a without view_psf (miss, hit), PSF b WITH view_psf (round the cache: psf_dev must hold b), a again (hit)
    a = Step(A_SHAPE, "A", 700, A_PSF, 20, -20, NO_PSF, inc=2, stream=5)
    b = Step(A_SHAPE, "A", 701, A_PSF, 20, -20, OUTPUTS, inc=2, stream=5)
    out += [a, a, b, a]
    # ---- the weight image cache: A -> C -> A, release_caches, A
    c = Step(C_SHAPE, "C", 702, C_PSF, 20, -20, NO_PSF, inc=2, stream=5)
    out += [a, c, a, RELEASE, a]
    return out


def n_iterations(steps) -> int:
    return sum(1 for s in steps if s is not RELEASE)


__all__ = ["Case", "Step", "cases", "landing", "TARGETS", "OUTPUTS", "SEED", "case_inputs", "phantom", "slab", "random_psf", "script", "volumes",
           "empty_planes", "n_iterations", "RELEASE", "A_SHAPE", "A_PSF", "F_SHAPE", "F_PSF", "C_SHAPE", "NO_PSF", "A_ANGLES"]
