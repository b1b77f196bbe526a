// The host side of the sparse tail (csrc/extract_plan.h) in a program of its own: plain g++ under ASan + UBSan, no HIP, no libmvsim.so.
//   1. the host condition (tail_sparse_caller, tail_sparse_ok) over all of its inputs, and tail_queue_sampler on the cases' shapes;
//   2. for every (nz, inc, Kz) of tests/test_skip_tail.py and of the flagship, strided and compact geometry: pass E skips buffer plane j
//      iff flag[j * zstride] is clear, the sampler's output plane k reads buffer plane k * g.inc and asks flag tail_flag_of_output -- the
//      flag of THAT plane, which is source plane k * inc, inside the array;
//   3. the vector form's slot walk (tail_slot_at / _next / _first, tail_lane) against plain divisions, for every wave of a grid.
// Prints "skip tail ok: <n> checks" on stderr; any failure returns 1.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "extract_plan.h"

using namespace mvsim;

static long checks = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        ++checks;                                                           \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

struct Case { int nz, ny, nx, kz; };
// (the shapes of the issue, the shapes tests/test_skip_tail.py runs them at -- wide enough for the fused rotate kernel --, the flagship)
static const Case kCases[] = {{24, 64, 64, 5}, {20, 77, 70, 7}, {24, 64, 72, 5}, {24, 128, 128, 5}, {20, 145, 139, 7}, {24, 144, 140, 5},
                              {16, 512, 512, 3}, {512, 512, 512, 31}};

static int condition()
{
    for (int m = 0; m < 32; ++m) {
        const bool has_flags = m & 1, skip_tail = m & 2, con = m & 4, fused = m & 8, queued = m & 16;
        const bool want = has_flags && skip_tail && !con && !fused && queued;
        CHECK(tail_sparse_ok(tail_sparse_caller(skip_tail, con, queued), has_flags, fused) == want);
    }
    for (const Case& c : kCases)
        for (int inc : {1, 3}) {
            const int64_t dim[3] = {c.nx, c.ny, c.nz};
            for (int share : {1, 5, 16, QUEUE_SHARE_AUTO, QUEUE_SHARE_AUTO + 7}) CHECK(tail_queue_sampler(dim, inc, true, QueueMode{share, nullptr}));
            CHECK(!tail_queue_sampler(dim, inc, true, QueueMode{0, nullptr}));          // poisson_queue = 0: the one-kernel samplers
            CHECK(!tail_queue_sampler(dim, inc, false, QueueMode{16, nullptr}));        // no noise: the copy forms
        }
    const int64_t tiny[3] = {15, 17, 8};                                               // a plane below a slot
    CHECK(!tail_queue_sampler(tiny, 1, true, QueueMode{16, nullptr}));
    return 0;
}

static int flags_of_planes()
{
    for (const Case& c : kCases)
        for (int inc : {1, 3})
            for (int compact = 0; compact < 2; ++compact) {
                const int64_t dim[3] = {c.nx, c.ny, c.nz};
                // a specimen in the middle planes, dilated by the taps' reach: the dilated flags the passes share
                std::vector<int> flag((size_t)c.nz, 0);
                for (int z = 0; z < c.nz; ++z) flag[(size_t)z] = (z >= c.nz / 2 - 1 - c.kz / 2 && z <= c.nz / 2 + 1 + c.kz / 2) ? 1 : 0;
                const ExtractGeom g = compact ? ExtractGeom::compact(dim, inc) : ExtractGeom::strided(dim, inc);
                const int zstride = compact ? inc : 1;                                  // (ConvTail::zstride as applied)
                const long long nk = (c.nz - 1) / zstride + 1;                          // planes pass E produces
                std::vector<int> stored((size_t)nk, 0), source((size_t)nk, 0);
                for (long long j = 0; j < nk; ++j) {
                    const long long f = tail_flag_of_buffer_plane(j, zstride);
                    CHECK(f >= 0 && f < c.nz);
                    stored[(size_t)j] = flag[(size_t)f];
                    source[(size_t)j] = (int)(j * zstride);
                }
                CHECK(g.nzo == (c.nz - 1) / inc + 1 && g.in_offset == 0);
                for (long long k = 0; k < g.nzo; ++k) {
                    const long long j = k * g.inc, f = tail_flag_of_output(g, k, zstride);
                    CHECK(j >= 0 && j < nk && f >= 0 && f < c.nz);
                    CHECK(f == k * inc && source[(size_t)j] == k * inc);               // the plane read IS source plane k * inc ...
                    CHECK(flag[(size_t)f] == stored[(size_t)j]);                       // ... and its flag the one pass E decided on
                    CHECK((long long)g.index_inc * k == f);                            // (the RNG counts in source planes too)
                }
            }
    return 0;
}

static int slot_walk()
{
    for (const Case& c : kCases)
        for (int inc : {1, 3}) {
            if ((c.nx * c.ny) % 4 != 0) continue;                                      // the group-by-group form has no plane boundary in a slot
            const int64_t dim[3] = {c.nx, c.ny, c.nz};
            const ExtractGeom g = ExtractGeom::compact(dim, inc);
            const ExtractPlan pl = extract_plan(g, true, true, QueueMode{16, nullptr});
            CHECK(pl.kernel == EXTRACT_K_NOISE2);
            const unsigned int p4 = (unsigned int)(g.plane / 4), total4 = (unsigned int)(g.plane / 4 * g.nzo);
            CHECK(p4 >= 64u && g.plane >= TAIL_SPARSE_MIN_PLANE);
            // the flagship's grid is 16384 blocks: every 61st block of it, all blocks of the small ones
            const unsigned int step = (unsigned int)pl.blocks * 256u, dq = step / p4, dr = step - dq * p4;
            for (unsigned int b = 0; b < (unsigned int)pl.blocks; b += (pl.blocks > 4096 ? 61u : 1u))
                for (unsigned int w = 0; w < 4u; ++w) {
                    unsigned int o0 = b * 256u + w * 64u;
                    TailSlot s = tail_slot_at(o0, p4);
                    for (; o0 < total4; o0 += step, s = tail_slot_next(s, dq, dr, p4)) {
                        CHECK(s.k == o0 / p4 && s.rem == o0 % p4);
                        const unsigned int first = tail_slot_first(s, p4);
                        CHECK(first >= 1u && (first >= 64u) == (o0 / p4 == (o0 + 63u) / p4));
                        const unsigned int lanes[6] = {0u, 1u, first - 1u, first, first + 1u, 63u};   // both sides of the plane boundary
                        for (unsigned int lane : lanes) {
                            if (lane >= 64u) continue;
                            const unsigned int o = o0 + lane;
                            const TailLane t = tail_lane(s, lane, p4);
                            CHECK(t.k == o / p4 && t.within == o % p4 && t.second == (t.k != s.k) && t.k <= s.k + 1u);
                            if (o < total4) CHECK(t.k < (unsigned int)g.nzo);
                            // the kernel's form of the lane's place in the buffer: the slot's first group + lane + the planes skipped at the boundary
                            for (unsigned int stride : {1u, (unsigned int)inc})
                                CHECK((unsigned long long)t.k * stride * p4 + t.within ==
                                      (unsigned long long)(s.k * stride) * p4 + s.rem + lane + (t.second ? (unsigned long long)(stride - 1u) * p4 : 0ull));
                        }
                    }
                }
        }
    return 0;
}

int main()
{
    if (condition() || flags_of_planes() || slot_walk()) return 1;
    std::fprintf(stderr, "skip tail ok: %ld checks\n", checks);
    return 0;
}
