// csrc/rotate_dev.h in a program of its own (host compiler, -O2 -ffp-contract=off, no HIP, no libmvsim.so), linked with the
// oracle's C restatement (oracle/mvsim_oracle.c): the one statement of the rotate kernels' arithmetic against the oracle.
//   volume Nx = 5, Ny = 37, Nz = 29; rotations about x by 0, 15, 33, -52, 90, 180 degrees.
// Every output voxel is computed twice -- as rot_value(...), the per-lane form of the rows the attenuation never visits, and
// as row_geometry + load_taps_masked + blend4, the form of the table kernels -- and both volumes must equal the oracle's
// rotateAroundAxis bit for bit.  attenuate_step then runs down every column (Nx steps from y = Ny - 1, as the kernels walk)
// and must equal the oracle's attenuate3d bit for bit for delta 0.01 and 0.4.  The rows of each kind (none / all four taps
// inside / partial) are counted and printed; at 33 degrees none of the three counts may be zero, so the masked path is not skipped.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mvsim_oracle.h"
#include "rotate_dev.h"

using namespace mvsim;

int main()
{
    const int nx = 5, ny = 37, nz = 29;
    const int64_t dim[3] = {nx, ny, nz};
    const long long row = nx, plane = (long long)nx * ny;
    const size_t nvox = (size_t)nx * ny * nz;
    std::vector<float> in(nvox), want(nvox), by_value(nvox), by_table(nvox), att_want(nvox), att_got(nvox);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (float& v : in) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        v = (float)((rng >> 40) + 1) * (4.0f / 16777216.0f);                 // (0, 4]
    }
    for (int deg : {0, 15, 33, -52, 90, 180}) {
        double m[12];
        Affine a;
        orc_axis_rotation(dim, 0, deg, m);
        orc_affine_invert(m, a.m);
        if (orc_rotate_around_axis(in.data(), dim, 0, deg, want.data()) != 0) return 1;
        long kinds[3] = {0, 0, 0};
        for (int z = 0; z < nz; ++z)
            for (int y = 0; y < ny; ++y) {
                const RowGeo g = row_geometry(a, y, (double)z, ny, nz, row);
                kinds[row_class(g.kind)] += 1;
                for (int x = 0; x < nx; ++x) {
                    float a00, a10, a11, a01;
                    load_taps_masked(in.data(), g, g.kind, true, x, row, plane, a00, a10, a11, a01);
                    by_table[x + row * y + plane * z] = blend4(a00, a10, a11, a01, g);
                    by_value[x + row * y + plane * z] = rot_value(in.data(), a, x, y, (double)z, nx, ny, nz);
                }
            }
        std::fprintf(stderr, "row geometry: %4d degrees: rows of kind 0 / 1 / partial: %ld / %ld / %ld\n", deg, kinds[0], kinds[1], kinds[2]);
        if (std::memcmp(by_value.data(), want.data(), nvox * sizeof(float)) != 0) {
            std::fprintf(stderr, "row geometry: rot_value differs from the oracle at %d degrees\n", deg);
            return 1;
        }
        if (std::memcmp(by_table.data(), want.data(), nvox * sizeof(float)) != 0) {
            std::fprintf(stderr, "row geometry: row_geometry + load_taps_masked + blend4 differ from the oracle at %d degrees\n", deg);
            return 1;
        }
        if (deg == 33 && (kinds[0] == 0 || kinds[1] == 0 || kinds[2] == 0)) {
            std::fprintf(stderr, "row geometry: a kind of row does not occur at 33 degrees\n");
            return 1;
        }
        for (double delta : {0.01, 0.4}) {
            if (orc_attenuate3d(want.data(), dim, delta, att_want.data()) != 0) return 1;
            std::fill(att_got.begin(), att_got.end(), 0.f);
            for (int z = 0; z < nz; ++z)
                for (int x = 0; x < nx; ++x) {
                    double n = 1.0;
                    for (int step = 0, y = ny - 1; step < nx; ++step, --y) {
                        const size_t i = x + row * y + plane * z;
                        att_got[i] = attenuate_step(n, want[i], delta);
                    }
                }
            if (std::memcmp(att_got.data(), att_want.data(), nvox * sizeof(float)) != 0) {
                std::fprintf(stderr, "row geometry: attenuate_step differs from the oracle at %d degrees, delta %g\n", deg, delta);
                return 1;
            }
        }
    }
    std::fprintf(stderr, "row geometry ok: 6 rotations\n");
    return 0;
}
