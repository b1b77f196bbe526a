// The trip walk of the vector sampler behind a sparse tail (csrc/extract_plan.h: tail_mask_*, tail_walk_aligned, tail_trips, TailSlot) held
// to plain divisions, in a program of its own: plain g++ under ASan + UBSan, no HIP, no libmvsim.so.  For every geometry below, inc 1..4,
// strided and compact, for the first wave, the last wave and about a thousand waves in between, and for every trip of each:
//   * the mask a refill builds -- the ballot over the 64 lanes' tail_mask_ask, emulated here -- has bit t = the flag of the plane trip t
//     starts in (found by division, its flag through tail_flag_of_output) and bit 32 + t = the flag of the plane behind it, clamped at the
//     last plane; bits of trips past the end of the output are clear;
//   * what the loop then reads from the mask it shifts (tail_mask_first / _second / _next) is the same, trip by trip, refills included;
//   * the carried slot is the divided one; the number of trips is the ceiling; behind the last trip no bit is left;
//   * tail_walk_aligned: no slot of such a geometry straddles a plane or is cut by the end of the output.
// Prints "tail walk ok: <n> checks" on stderr; any failure returns 1.
#include <cstdint>
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

struct Geometry { int nz, ny, nx; unsigned int trips_inc1; };   // trips of the first wave at inc 1
static const Geometry kGeometries[] = {
    {512, 512, 512, 8},        // the flagship
    {1024, 1024, 1024, 64},    // one refill
    {512, 2048, 2048, 128},    // 2^31 outputs: three refills
    {68, 512, 512, 2},         // tests/test_tail_walk.py: aligned, two trips
    {72, 510, 508, 2},         // ... straddling (64 770 groups per plane), two trips
    {24, 144, 140, 1},         // 5 040 groups x 24 planes: one trip
};

// one wave's walk; flag: the dilated flags per SOURCE plane
static int walk_wave(const ExtractGeom& g, int zstride, const std::vector<int>& flag, unsigned int o_first, unsigned int step, unsigned int p4,
                     unsigned int total4, bool aligned)
{
    const unsigned int klast = (unsigned int)g.nzo - 1u;
    auto flag_of = [&](unsigned int k) { return flag.at((size_t)tail_flag_of_output(g, (long long)k, zstride)) != 0; };
    const unsigned int dq = step / p4, dr = step % p4;
    unsigned int o0 = o_first, trip = 0u;
    TailSlot sl = tail_slot_at(o0, p4);
    unsigned long long mask = 0ull;
    for (; o0 < total4; ++trip) {
        if (tail_mask_refill(trip)) {
            CHECK(trip % 32u == 0u && mask == 0ull);                               // the old mask is used up, bit for bit
            for (unsigned int lane = 0; lane < 64u; ++lane) {                      // the ballot
                const TailAsk a = tail_mask_ask(o0, lane, step, p4, total4, klast);
                const unsigned long long ot = (unsigned long long)o0 + (unsigned long long)(lane % 32u) * step;
                CHECK(a.ask == (ot < total4));
                if (!a.ask) continue;
                const unsigned int kt = (unsigned int)(ot / p4);
                CHECK(kt <= klast && a.k == (lane < 32u ? kt : (kt < klast ? kt + 1u : klast)));
                if (flag_of(a.k)) mask |= 1ull << lane;
            }
        } else {
            CHECK(trip % 32u != 0u);
        }
        const unsigned int k = o0 / p4, rem = o0 % p4;
        CHECK(sl.k == k && sl.rem == rem && k <= klast);
        CHECK(tail_mask_first(mask) == flag_of(k));
        CHECK(tail_mask_second(mask) == flag_of(k < klast ? k + 1u : klast));      // the clamp: a slot in the last plane has no second one
        if (aligned) CHECK(rem % 64u == 0u && tail_slot_first(sl, p4) >= 64u && o0 + 63u < total4);
        o0 += step; sl = tail_slot_next(sl, dq, dr, p4); mask = tail_mask_next(mask);
    }
    const unsigned long long span = (unsigned long long)total4 - o_first;
    const unsigned int ceiling = o_first < total4 ? (unsigned int)((span + step - 1u) / step) : 0u;
    CHECK(trip == ceiling && tail_trips(o_first, total4, step) == ceiling);
    // no bit past the last trip: what is left of the mask behind it belongs to trips that do not exist
    CHECK(mask == 0ull);
    return 0;
}

static int geometry(const Geometry& c, int inc, bool compact)
{
    const int64_t dim[3] = {c.nx, c.ny, c.nz};
    const ExtractGeom g = compact ? ExtractGeom::compact(dim, inc) : ExtractGeom::strided(dim, inc);
    const int zstride = compact ? inc : 1;
    const ExtractPlan pl = extract_plan(g, true, true, QueueMode{16, nullptr});
    CHECK(pl.kernel == EXTRACT_K_NOISE2 && g.plane % 4 == 0 && g.plane * g.nzo < (1ll << 32));
    const unsigned int p4 = (unsigned int)(g.plane / 4), total4 = (unsigned int)(g.plane / 4 * g.nzo), step = (unsigned int)pl.blocks * 256u;
    const bool aligned = tail_walk_aligned(p4);
    CHECK(aligned == (p4 % 64u == 0u) && p4 >= 64u);
    if (inc == 1) CHECK(tail_trips(0u, total4, step) == c.trips_inc1);
    // flags per source plane: a hash, so that neighbouring planes differ often and runs of both values occur
    std::vector<int> flag((size_t)c.nz);
    for (int z = 0; z < c.nz; ++z) flag[(size_t)z] = (int)((((unsigned int)z * 2654435761u) >> 29) < 5u) * (1 + z % 3);   // non-zero values other than 1 too
    const unsigned int waves = (unsigned int)pl.blocks * 4u;
    const unsigned int stride = waves > 1000u ? (waves / 1000u) | 1u : 1u;
    for (unsigned int w = 0; w < waves; w += stride) CHECK(walk_wave(g, zstride, flag, (w / 4u) * 256u + (w % 4u) * 64u, step, p4, total4, aligned) == 0);
    CHECK(walk_wave(g, zstride, flag, ((waves - 1u) / 4u) * 256u + ((waves - 1u) % 4u) * 64u, step, p4, total4, aligned) == 0);
    return 0;
}

int main()
{
    static_assert(TAIL_MASK_TRIPS == 32u, "the masks of a slot's two planes are the halves of one 64-lane ballot");
    for (const Geometry& c : kGeometries)
        for (int inc = 1; inc <= 4; ++inc)
            for (int compact = 0; compact < 2; ++compact)
                if (geometry(c, inc, compact != 0)) {
                    std::fprintf(stderr, "  in (nz, ny, nx) = (%d, %d, %d), inc %d, %s\n", c.nz, c.ny, c.nx, inc, compact ? "compact" : "strided");
                    return 1;
                }
    std::fprintf(stderr, "tail walk ok: %ld checks\n", checks);
    return 0;
}
