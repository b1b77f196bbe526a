// csrc/extract_plan.h in a program of its own (plain g++, no HIP, no libmvsim.so): geometry requests on stdin, one per line,
//     <kind> nx ny nz inc a b c aligned16 noise share
// kind strided / compact: ExtractGeom::strided / compact(dim, inc); slab: ExtractGeom::slab(dim, inc, z0 = a, z1 = b, compact = c);
// path: what mvsim_extract_path plans -- strided(dim, inc) on RNG plane stride a (0: inc) from counter b.  Answer, one line each:
//     plane nzo inc index_inc index_offset in_offset  kernel checked blocks segcap full_items slots_per_plane share  counts_bytes total_bytes
// tests/test_poisson_sweep.py holds the answers to the case list and to the built library.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "extract_plan.h"

int main()
{
    char kind[16];
    long long nx, ny, nz, a, c;
    unsigned long long b;
    int inc, aligned16, noise, share;
    long lines = 0;
    while (std::scanf("%15s %lld %lld %lld %d %lld %llu %lld %d %d %d", kind, &nx, &ny, &nz, &inc, &a, &b, &c, &aligned16, &noise, &share) == 11) {
        const int64_t dim[3] = {nx, ny, nz};
        mvsim::ExtractGeom g;
        if (!std::strcmp(kind, "strided")) g = mvsim::ExtractGeom::strided(dim, inc);
        else if (!std::strcmp(kind, "compact")) g = mvsim::ExtractGeom::compact(dim, inc);
        else if (!std::strcmp(kind, "slab")) g = mvsim::ExtractGeom::slab(dim, inc, a, (int64_t)b, c != 0);
        else if (!std::strcmp(kind, "path")) {
            g = mvsim::ExtractGeom::strided(dim, inc);
            if (a > 0) g.index_inc = (int)a;
            g.index_offset = b;
        } else {
            std::fprintf(stderr, "unknown request '%s'\n", kind);
            return 2;
        }
        const mvsim::ExtractPlan p = mvsim::extract_plan(g, aligned16 != 0, noise != 0, mvsim::QueueMode{share, nullptr});
        std::printf("%lld %lld %d %d %" PRIu64 " %lld  %d %d %d %u %u %lld %d  %zu %zu\n", p.geom.plane, p.geom.nzo, p.geom.inc, p.geom.index_inc,
                    p.geom.index_offset, p.geom.in_offset, p.kernel, p.checked ? 1 : 0, p.blocks, p.segcap, p.full_items, p.slots_per_plane, p.share,
                    p.layout.counts_bytes, p.layout.total_bytes);
        lines += 1;
    }
    if (!std::feof(stdin)) { std::fprintf(stderr, "malformed request after %ld lines\n", lines); return 2; }
    std::fprintf(stderr, "extract plan run ok: %ld requests\n", lines);
    return 0;
}
