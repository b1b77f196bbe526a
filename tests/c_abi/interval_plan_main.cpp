// csrc/interval_plan.h under plain g++ (tests/test_intervals_host.py builds this with -fsanitize=address,undefined and runs it as a child
// process): no HIP, no libmvsim.so.  Requests on stdin, one per line; one line of integers per request on stdout.
//   geom Nx Ny Nz  x0 y0 z0  x1 y1 z1  inc noise share
//        -> ok tx ty tz nzo n_out row_pitch plane_pitch in_offset kernel checked blocks segcap slots_per_plane queue_bytes   (ok = 1)
//        -> 0                                                                                                            (refused)
//   tile Nx Ny Nz  r0 r1 r2  tile      (ratios as decimal fractions)
//        -> min[3] max[3] overlap[3]
//   same tx ty tz inc noise snr_bits   tx ty tz inc noise snr_bits
//        -> 1 when the two jobs share launches
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "interval_plan.h"

using namespace mvsim;

int main()
{
    std::string line;
    long n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "geom") {
            int64_t dim[3], mn[3], mx[3];
            int inc, noise, share;
            is >> dim[0] >> dim[1] >> dim[2] >> mn[0] >> mn[1] >> mn[2] >> mx[0] >> mx[1] >> mx[2] >> inc >> noise >> share;
            if (!is) { std::fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
            IntervalGeom g;
            if (interval_geom(dim, mn, mx, inc, &g) != nullptr) { std::printf("0\n"); ++n; continue; }
            const IntervalPlan p = interval_plan(g, noise != 0, QueueMode{share, nullptr});
            // the tile is planned as a zero-min volume: its counters start at 0 and advance by inc planes of the TILE
            if (p.xp.geom.plane != (long long)g.tile[0] * g.tile[1] || p.xp.geom.index_offset != 0 || p.xp.geom.index_inc != inc ||
                p.xp.geom.in_offset != g.in_offset || p.xp.geom.nzo != g.nzo()) {
                std::fprintf(stderr, "plan does not describe the zero-min tile: %s\n", line.c_str());
                return 3;
            }
            std::printf("1 %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d %u %lld %zu\n", (long long)g.tile[0], (long long)g.tile[1], (long long)g.tile[2],
                        g.nzo(), g.n_out(), g.row_pitch, g.plane_pitch, g.in_offset, p.xp.kernel, p.xp.checked ? 1 : 0, p.xp.blocks, p.xp.segcap,
                        p.xp.slots_per_plane, p.xp.layout.total_bytes);
        } else if (what == "tile") {
            int64_t dim[3], mn[3], mx[3], ov[3];
            double r[3];
            int tile;
            is >> dim[0] >> dim[1] >> dim[2] >> r[0] >> r[1] >> r[2] >> tile;
            if (!is) { std::fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
            tile_interval(dim, r, tile, mn, mx, ov);
            std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)mn[0], (long long)mn[1], (long long)mn[2], (long long)mx[0],
                        (long long)mx[1], (long long)mx[2], (long long)ov[0], (long long)ov[1], (long long)ov[2]);
        } else if (what == "same") {
            IntervalKey k[2];
            for (IntervalKey& q : k) {
                int noise;
                is >> q.tile[0] >> q.tile[1] >> q.tile[2] >> q.inc >> noise >> q.snr_bits;
                q.noise = noise != 0;
            }
            if (!is) { std::fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
            std::printf("%d\n", k[0] == k[1] ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown request: %s\n", line.c_str());
            return 2;
        }
        ++n;
    }
    std::fprintf(stderr, "interval plan run ok: %ld requests\n", n);
    return 0;
}
