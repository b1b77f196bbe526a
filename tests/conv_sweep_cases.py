"""Deterministic cases of the convolution sweep (tests/test_conv_sweep.py): every length of the hand-written FFT's size table in
every role it plays, every instance of the direct stencil and the direct z pass, the split y lines, the fused rotate + attenuate
+ x transform and the sizes just past the table.  Pure Python: the CPU tests check the table, the coverage and the yardstick's
sensitivity from the same list the GPU tests run.

Shapes are (x, y, z) here, as the library counts them; numpy volumes are (z, y, x)."""
from __future__ import annotations

from dataclasses import dataclass, field

# The product branch of MVSIM_FFT_SIZES (csrc/fft_dev.h), restated: (L, radices).
FFT_SIZES = [
    (16, (4, 4)), (18, (9, 2)), (20, (5, 4)), (24, (3, 8)), (32, (4, 8)), (36, (9, 4)), (40, (5, 8)), (48, (3, 4, 4)),
    (56, (7, 8)), (64, (8, 8)), (72, (9, 8)), (80, (5, 4, 4)), (96, (3, 8, 4)), (112, (7, 4, 4)), (128, (4, 8, 4)),
    (140, (7, 5, 4)), (144, (9, 4, 4)), (160, (5, 8, 4)), (180, (9, 5, 4)), (192, (3, 8, 8)), (224, (7, 8, 4)),
    (256, (4, 8, 8)), (280, (7, 5, 8)), (288, (9, 8, 4)), (320, (5, 8, 8)), (350, (7, 10, 5)), (360, (9, 5, 8)),
    (384, (3, 8, 4, 4)), (448, (7, 8, 8)), (512, (8, 8, 8)), (540, (9, 5, 4, 3)), (560, (7, 8, 10)), (576, (9, 8, 8)),
    (640, (5, 8, 4, 4)), (720, (9, 8, 10)), (768, (3, 8, 8, 4)), (896, (7, 8, 4, 4)), (1024, (4, 8, 8, 4)),
    (1080, (9, 8, 5, 3)), (1120, (7, 8, 5, 4)), (1152, (9, 8, 4, 4)), (1280, (5, 8, 8, 4)), (1440, (9, 8, 5, 4)),
    (1536, (3, 8, 8, 8)), (1792, (7, 8, 8, 4)), (2048, (8, 8, 8, 4)), (2160, (10, 8, 9, 3)), (2240, (7, 8, 8, 5)),
]
LENGTHS = [L for L, _ in FFT_SIZES]
SPLIT_LENGTHS = (2048, 2160, 2240)        # y lines taken as two half-length transforms (k_fft_lines_split: 1024, 1080, 1120)
FUSED_RANGE = (72, 576)                   # half lengths k_rotate_attenuate_fftx is instantiated for (rot_fftx_len_ok)
MAX_MACS = 7e7                            # multiply-adds of the fp64 reference per case


def prev_len(L: int) -> int:
    """The table entry below L (1 below the first: the smallest need that still lands on it)."""
    i = LENGTHS.index(L)
    return LENGTHS[i - 1] if i else 1


def pick(need: int) -> int | None:
    """custom_fft_sizes' rule for y and z: the smallest entry >= need (None past the table)."""
    for L in LENGTHS:
        if L >= need:
            return L
    return None


def pick_x(need: int) -> int | None:
    """... and for x: the half length M = smallest entry >= ceil(need / 2); Px = 2 M."""
    return pick((need + 1) // 2)


def lines_per_tile(L: int) -> int:
    """Cfg<L>::NL: 16 lines per block up to 576 points, 8 above."""
    return 16 if L <= 576 else 8


NLZ = 16                                  # columns of a direct z pass tile (fft_host.h)


def hxp(px: int, py: int, pz: int, zdirect: bool) -> int:
    """Complex row pitch of the spectrum (custom_fft_geometry)."""
    M = px // 2
    tw = max(lines_per_tile(py), NLZ if zdirect else lines_per_tile(pz))
    return (M + 1 + tw - 1) // tw * tw


def split_taken(dim, kdim, zpass: str = "auto", exp: int = 0) -> bool:
    """Whether the image's y passes take k_fft_lines_split (launch_lines): a split length, exp bit 8 clear and an even number of
    8-column tiles.  (The mirrored-row condition there is the one the direct z pass's mirrored y halo already meets.)"""
    px, py = 2 * pick_x(dim[0] + kdim[0] - 1), pick(dim[1] + kdim[1] - 1)
    zdirect = zpass != "fft" and kdim[2] <= 64
    pz = pick(dim[2] + kdim[2] - 1) if not zdirect else 16
    if py not in SPLIT_LENGTHS or exp & 8:
        return False
    return (hxp(px, py, pz, zdirect) // lines_per_tile(py)) % 2 == 0


# ---------------------------------------------------------------------------------------- the direct stencil's geometry
STENCIL_TX, STENCIL_PTY, STENCIL_PTZ = 32, 16, 8


def stencil_geometry(kdim):
    """pair_geometry (stencil.hip), restated: (x taps of a chunk = 4 NG, kyc, kzc).  The CPU test holds it to the library's
    mvsim_stencil_geometry."""
    kx, ky, kz = kdim
    assert 1 <= min(kdim) and max(kdim) <= 64
    budget = 78 * 1024
    best, res = 1e300, None
    for ng in range(1, (kx + 3) // 4 + 1):
        kxp = 4 * ng
        s2 = (STENCIL_TX + kxp - 1) | 1
        xchunks = (kx + kxp - 1) // kxp
        for kyc in range(1, ky + 1):
            for kzc in range(1, kz + 1):
                if 8 * s2 * (7 + kyc) * (STENCIL_PTZ - 1 + kzc) > budget:
                    break
                chunks = float(xchunks) * ((ky + kyc - 1) // kyc) * ((kz + kzc - 1) // kzc)
                rows = float(15 + kyc) * (STENCIL_PTZ - 1 + kzc)
                fill = rows / 16.0 * 2500.0 + rows / 4.0 * 40.0 + 3000.0
                cost = chunks * fill + float(xchunks) * ky * kz * (150.0 + (kxp * 8 // 2) * 4.0)
                if cost < best:
                    best, res = cost, (kxp, kyc, kzc)
    return res


def stencil_near(dim, kdim) -> bool:
    """launch_stencil's NEAR instance: one reflection reaches every halo index (N >= tile + K per axis, x padded taps included)."""
    kxp = stencil_geometry(kdim)[0]
    return (dim[0] >= STENCIL_TX + kdim[0] + kxp and dim[1] >= STENCIL_PTY + kdim[1] and dim[2] >= STENCIL_PTZ + kdim[2])


# ---------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    role: str                  # ylines | xpass | zfft | zfft_deep | split | fallback | zdirect | stencil | fused
    dim: tuple                 # (Nx, Ny, Nz)
    kdim: tuple                # (Kx, Ky, Kz)
    target: dict               # what the case lands on: L / M / NG, NEAR / G / ...
    opts: dict = field(default_factory=dict)
    method: int = 1
    tag: str = ""

    @property
    def id(self) -> str:
        t = "-".join(f"{k}{v}" for k, v in self.target.items())
        o = "".join(f"-{k}={v}" for k, v in self.opts.items())
        return f"{self.role}-{t}{o}{'-' + self.tag if self.tag else ''}-{'x'.join(map(str, self.dim))}-k{'x'.join(map(str, self.kdim))}"

    @property
    def shape(self):           # numpy (z, y, x)
        return self.dim[::-1]

    @property
    def kshape(self):
        return self.kdim[::-1]

    @property
    def macs(self) -> int:
        n = self.dim[0] * self.dim[1] * self.dim[2]
        return n * self.kdim[0] * self.kdim[1] * self.kdim[2]

    def padded(self):
        """(Px, Py, Pz) of custom_fft_sizes, or None past the table."""
        m, py, pz = pick_x(self.dim[0] + self.kdim[0] - 1), pick(self.dim[1] + self.kdim[1] - 1), pick(self.dim[2] + self.kdim[2] - 1)
        if m is None or py is None or pz is None:
            return None
        return 2 * m, py, pz


def _small(i: int, lo: int, hi: int) -> int:
    """A deterministic value in [lo, hi] that moves with i (the axes a case does not target)."""
    return lo + (i * 7 + 3) % (hi - lo + 1)


def _with_parity(k: int, odd: bool) -> int:
    return k if (k % 2 == 1) == odd else k + 1


def _ylines():
    out = []
    for i, L in enumerate(LENGTHS):
        for slack, need in (("zero", L), ("max", prev_len(L) + 1)):
            odd = (i + (slack == "max")) % 2 == 0
            ky = min(_with_parity(3 + (i * 5) % 30, odd), need)
            if need == 1:
                ky = 1
            ny = need - ky + 1
            nx, kx = _small(i, 5, 14), _small(i + 1, 1, 4)
            nz, kz = _small(i + 2, 3, 7), _small(i, 1, 3)
            while nx * ny * nz * kx * ky * kz > 4e7 and nx > 3:
                nx -= 1
            out.append(Case("ylines", (nx, ny, nz), (kx, ky, kz), {"L": L, "slack": slack}))
    return out


def _xpass():
    out = []
    for i, M in enumerate(LENGTHS):
        # need = 2M, Nx even (Kx odd);  need = 2 prev(M) + 1 (odd), Kx even (Nx even)
        for slack, need, kodd in (("zero", 2 * M, True), ("max", 2 * prev_len(M) + 1, False)):
            kx = _with_parity(1 + (i * 3) % 32, kodd)
            kx = min(kx, need - 1) if kodd else min(kx, need - 1)
            if (need - kx + 1) % 2:
                kx -= 1
            nx = need - kx + 1
            assert nx % 2 == 0 and kx >= 1, (M, need, kx)
            ny, ky = _small(i, 3, 8), _small(i + 1, 1, 4)
            nz, kz = _small(i + 3, 2, 6), _small(i + 2, 1, 3)
            while nx * ny * nz * kx * ky * kz > 4e7 and ny > 2:
                ny -= 1
            out.append(Case("xpass", (nx, ny, nz), (kx, ky, kz), {"M": M, "slack": slack}))
    return out


def _zfft():
    out = []
    for i, L in enumerate(LENGTHS):
        kz = _with_parity(2 + (i * 3) % 25, i % 2 == 0)
        kz = min(kz, L)
        nz = L - kz + 1
        nx, kx = _small(i, 4, 11), _small(i + 2, 1, 4)
        ny, ky = _small(i + 1, 3, 9), _small(i + 3, 1, 3)
        while nx * ny * nz * kx * ky * kz > 4e7 and nx > 2:
            nx -= 1
        out.append(Case("zfft", (nx, ny, nz), (kx, ky, kz), {"L": L}, opts={"fft_zpass": "fft"}))
        if L >= 128:
            # more than 64 z taps: the FFT z pass without the option; need anywhere in (prev, L]
            kz = 65 + (i * 11) % 40
            need = L - (i % 3) * (L - prev_len(L) - 1) // 2
            nz = need - kz + 1
            if nz < 2:
                nz, kz = 2, need - 1
            nx, kx = _small(i, 3, 7), _small(i + 1, 1, 3)
            ny, ky = _small(i + 2, 3, 7), _small(i, 1, 3)
            while nx * ny * nz * kx * ky * kz > 4e7 and ny > 2:
                ny -= 1
            while nx * ny * nz * kx * ky * kz > 4e7 and nx > 2:
                nx -= 1
            out.append(Case("zfft_deep", (nx, ny, nz), (kx, ky, kz), {"L": L}))
    return out


def _split():
    out = []
    for j, L in enumerate(SPLIT_LENGTHS):
        p = prev_len(L)
        # taken: the direct z pass (hxp a multiple of 16, an even number of 8-column tiles)
        ky = 13 + 6 * j
        ny = L - ky + 1 - 3 * j
        out.append(Case("split", (6 + j, ny, 4 + j), (3, ky, 2 + j), {"L": L, "form": "split"}))
        # declined: the FFT z pass on more than 576 points (8-line z tiles) and a half length of 16 (hxp 24: three tiles)
        ky = 4 + j
        ny = p + 1 - ky + 1 + 5 * j
        out.append(Case("split", (2, ny, 576), (1, ky, 3), {"L": L, "form": "declined"}, opts={"fft_zpass": "fft"}))
    return out


def _fallback():
    return [Case("fallback", (4, 2241 - 40, 4), (3, 41, 2), {"need": "y2241"}),
            Case("fallback", (4481 - 30, 3, 3), (31, 2, 1), {"need": "x4481"})]


def _zdirect():
    out = []
    for kz in range(1, 65):
        # Nz a multiple of the 16-plane z unit, or not; now and then thinner than the PSF
        nz = 16 * (1 + kz % 4) if kz % 2 else 16 * (kz % 3) + 1 + (kz * 5) % 15
        if kz % 7 == 3:
            nz = max(2, kz // 2)
        nx, kx = _small(kz, 6, 20), _small(kz + 1, 1, 4)
        ny, ky = _small(kz + 2, 5, 14), _small(kz + 3, 1, 4)
        out.append(Case("zdirect", (nx, ny, nz), (kx, ky, kz), {"Kz": kz}))
    return out


def _stencil_chunk_edges(kx: int):
    """(ky, kz) pairs whose last y or z chunk is full (K = a multiple of the chunk) or one tap long (K = chunk + 1), for x taps
    kx: the smallest PSF of each kind."""
    found = {}
    def near_macs(t):
        ky, kz = t
        return (STENCIL_TX + 2 * kx + 3) * (STENCIL_PTY + ky) * (STENCIL_PTZ + kz) * kx * ky * kz

    for ky, kz in sorted(((a, b) for a in range(2, 65) for b in range(2, 65)), key=lambda t: (near_macs(t), t)):
        _, kyc, kzc = stencil_geometry((kx, ky, kz))
        for axis, k, kc in (("y", ky, kyc), ("z", kz, kzc)):
            if kc < k and k % kc in (0, 1):
                found.setdefault(f"{axis}_{'full' if k % kc == 0 else 'plus1'}", (ky, kz))
        if len(found) == 4:
            break
    return found


def _stencil():
    out = []
    for ng in range(1, 17):
        for kx in (4 * ng, 4 * ng - 3):
            ky, kz = 1 + ng % 3, 1 + (ng + kx) % 3
            for near in (True, False):
                kxp = 4 * ng
                if near:
                    dim = (STENCIL_TX + kx + kxp + ng % 5, STENCIL_PTY + ky + ng % 3, STENCIL_PTZ + kz + ng % 2)
                else:
                    # thin in y and z (more than one reflection), x not a multiple of the tile
                    dim = (kx + 5 + (ng % 4) * 7, 3 + ng % 5, 2 + ng % 3)
                out.append(Case("stencil", dim, (kx, ky, kz), {"NG": ng, "NEAR": int(near)}, method=2))
    # chunk boundaries along y and z: K = a multiple of the chunk, K = chunk + 1
    for kx in (2,):
        for edge, (ky, kz) in sorted(_stencil_chunk_edges(kx).items()):
            kxp = stencil_geometry((kx, ky, kz))[0]
            for near in (True, False):
                dim = ((STENCIL_TX + kx + kxp, STENCIL_PTY + ky, STENCIL_PTZ + kz) if near else (kx + 11, 9, 7))
                c = Case("stencil", dim, (kx, ky, kz), {"NG": kxp // 4, "NEAR": int(near)}, method=2, tag=edge)
                out.append(c)
    return out


def fused_geometry_ok(dim, kdim) -> bool:
    """rotate_attenuate_fftx's own conditions (besides rotation about x and option fused_fftx = 1)."""
    nx, ny, nz = dim
    kx, ky, kz = kdim
    if kz > 64 or not (ny > 1 and ky // 2 < ny and ky - 1 - ky // 2 < ny):
        return False
    if nx > 1024 or nx < 64 or kx > nx or nx > ny:
        return False
    m = pick_x(nx + kx - 1)
    return m is not None and FUSED_RANGE[0] <= m <= FUSED_RANGE[1]


def _fused():
    out = []
    ms = [M for M in LENGTHS if FUSED_RANGE[0] <= M <= FUSED_RANGE[1]]
    for i, M in enumerate(ms):
        p = prev_len(M)
        # G = 1 (<= 8 waves, Nx <= 512) wherever the half length is reachable with it
        for g in (1, 2):
            lo_need, hi_need = 2 * p + 1, 2 * M          # needs that land on M
            if g == 1:
                nx = min(512, hi_need) - (i * 13) % 40
                if nx % 64 == 0:
                    nx -= 3
                kx = max(1, lo_need - nx + 1 + (i % 5))
                if nx < 64 or kx > nx or nx + kx - 1 > hi_need:
                    continue
            else:
                if hi_need <= 512:
                    continue
                nx = max(513, lo_need - 20) + (i * 29) % 60
                nx = min(nx, 1024, hi_need)
                if nx % 64 == 0:
                    nx -= 1
                kx = max(1, lo_need - nx + 1)
                kx = max(kx, 1 + (i * 3) % 9)
                if nx + kx - 1 > hi_need:
                    kx = hi_need - nx + 1
            ny = nx + (0 if i % 3 == 0 else 5 + (i * 17) % 90)
            ky, kz = 3 + (i * 2) % 9, 3 + (i * 5) % 13
            nz = 2 + i % 3
            c = Case("fused", (nx, ny, nz), (kx, ky, kz), {"M": M, "G": g}, opts={"fused_fftx": 1}, tag=f"deg{(i * 37) % 180 - 90}")
            assert fused_geometry_ok(c.dim, c.kdim), c.id
            out.append(c)
    return out


def fused_degrees(case: Case) -> int:
    return int(case.tag[3:])


def fused_g(case: Case) -> int:
    """G of launch_rot_fftx_t: 2 when the row takes more than 8 waves."""
    return 2 if (case.dim[0] + 63) // 64 > 8 else 1


def cases():
    """Every case of the sweep, in a fixed order."""
    return _ylines() + _xpass() + _zfft() + _split() + _fallback() + _zdirect() + _stencil() + _fused()


def conv_cases():
    """The cases compared with the exact direct sum (all but the fused ones, which are compared bit for bit)."""
    return [c for c in cases() if c.role != "fused"]
