// csrc/sphere_walk.h on the CPU: the chunked resolution of the drawSpheres / multiSpheres walk -- per-position codes from a window of
// states, sorted event lists, chunk maps per entry offset, composition, emission with the true entries -- against a plain serial walk
// over java.util.Random written here.  No HIP, no libmvsim.so.
#include "sphere_walk.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mvsim;

namespace {

// ---- the serial walk, written from the JDK's specification of java.util.Random ------------------------------------------------------
const uint64_t MASK = (1ULL << 48) - 1, MUL = 0x5DEECE66DULL, ADD = 0xBULL;

struct Rnd {
    uint64_t s;
    long steps = 0;
    int next(int bits)
    {
        s = (s * MUL + ADD) & MASK;
        steps += 1;
        return (int)((int64_t)s >> (48 - bits));
    }
    int nextInt(int bound)
    {
        int r = next(31);
        const int m = bound - 1;
        if ((bound & m) == 0) return (int)(((int64_t)bound * (int64_t)r) >> 31);
        for (int u = r; (int)((unsigned)u - (unsigned)(r = u % bound) + (unsigned)m) < 0; u = next(31)) {}
        return r;
    }
    double nextDouble() { const int64_t hi = (int64_t)next(26) << 27; return (double)(hi + next(27)) * 0x1.0p-53; }
};

struct Accepted {
    int64_t ordinal;
    int raw;
    double value;
};

struct Serial {
    std::vector<Accepted> items;
    uint64_t end_state;
    long steps;
    std::vector<int> f;                 // steps per voxel
};

Serial serial_walk(uint64_t s0, int64_t n, int kind, int scale)
{
    Serial out;
    Rnd rnd{s0};
    const int64_t modulus = (int64_t)(7 * scale) * (7 * scale) * (7 * scale);
    for (int64_t i = 0; i < n; ++i) {
        const long before = rnd.steps;
        const int raw = rnd.nextInt(10 * scale);
        const double rv = rnd.nextDouble();
        bool take;
        if (kind == SW_RULE_DRAW) take = (int64_t)std::floor(rv * 10000 + 0.5) % modulus == 0;
        else take = rv * 100000 < 1;
        if (take) out.items.push_back(Accepted{i, raw, rnd.nextDouble()});
        out.f.push_back((int)(rnd.steps - before));
    }
    out.end_state = rnd.s;
    out.steps = rnd.steps;
    return out;
}

// ---- the chunked walk: what the three kernels do, one chunk after the other ---------------------------------------------------------
struct Chunked {
    bool fail = false, reached = false;
    std::vector<WalkEntry> entries;
    uint64_t end_state = 0;
    int64_t end_pos = -1;
};

Chunked chunked_walk(uint64_t s0, int64_t n, const WalkRule& rule, int P, int E, int max_events, int group)
{
    Chunked out;
    const int64_t cover = walk_cover(n);                // what the library covers
    const int64_t nchunks = (cover + P - 1) / P;
    std::vector<std::vector<uint32_t>> events((size_t)nchunks);
    std::vector<uint32_t> maps((size_t)nchunks * E);
    for (int64_t c = 0; c < nchunks; ++c) {
        uint64_t w[6];
        w[0] = jr_jump(s0, (uint64_t)(c * P));
        for (int i = 1; i < 6; ++i) w[i] = (w[i - 1] * JR_A + JR_C) & JR_MASK;
        bool chunk_fail = false;
        for (int q = 0; q < P; ++q) {
            const uint32_t code = walk_code(w, rule);
            if (code != 3u) {
                if ((int)events[c].size() < max_events) events[c].push_back(walk_event(q, code));
                else chunk_fail = true;
            }
            for (int i = 0; i < 5; ++i) w[i] = w[i + 1];
            w[5] = (w[5] * JR_A + JR_C) & JR_MASK;
        }
        for (int e = 0; e < E; ++e) maps[c * E + e] = walk_resolve(events[c].data(), (int)events[c].size(), P, e, E, chunk_fail).pack();
    }
    // the scan: runs of `group` chunks composed for every entry, then stitched, then every run again with its true entry
    std::vector<int> entry((size_t)nchunks);
    std::vector<int64_t> vbase((size_t)nchunks), abase((size_t)nchunks);
    std::vector<int> fail_at((size_t)nchunks);
    int e = 0, fail = 0;
    int64_t v = 0, a = 0;
    for (int64_t r0 = 0; r0 < nchunks; r0 += group) {
        const int64_t r1 = r0 + group < nchunks ? r0 + group : nchunks;
        std::vector<WalkMap> cur((size_t)E);
        for (int k = 0; k < E; ++k) { cur[k].exit = k; cur[k].fail = 0; cur[k].count = 0; cur[k].accepted = 0; }
        for (int64_t c = r0; c < r1; ++c)
            for (int k = 0; k < E; ++k) cur[k] = walk_compose(cur[k], WalkMap::unpack(maps[c * E + cur[k].exit]));
        int ee = e, ff = fail;
        int64_t vv = v, aa = a;
        for (int64_t c = r0; c < r1; ++c) {
            entry[c] = ee; vbase[c] = vv; abase[c] = aa;
            const WalkMap m = WalkMap::unpack(maps[c * E + ee]);
            ff |= m.fail;
            fail_at[c] = ff;
            vv += m.count; aa += m.accepted; ee = m.exit;
        }
        // the run's composed map must say what the chunk-by-chunk walk said (associativity)
        if (!cur[e].fail && !ff && (cur[e].exit != ee || v + cur[e].count != vv || a + cur[e].accepted != aa)) {
            std::fprintf(stderr, "composition of a run differs from the walk over its chunks\n");
            std::exit(2);
        }
        e = ee; fail = ff; v = vv; a = aa;
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        const WalkMap m = WalkMap::unpack(maps[c * E + entry[c]]);
        if (vbase[c] < n && vbase[c] + m.count >= n) {
            out.reached = true;
            out.fail = fail_at[c] != 0;
            if (out.fail) return out;
            for (int64_t k = 0; k <= c; ++k) {
                int64_t end = -1, at = abase[k];
                walk_chunk(events[k].data(), (int)events[k].size(), P, entry[k], vbase[k], n, &end, [&](int64_t ordinal, int q) {
                    const WalkVoxel vx = walk_voxel(jr_jump(s0, (uint64_t)(k * P + q)), rule);
                    if ((int64_t)out.entries.size() != at) { std::fprintf(stderr, "output base of chunk %lld is off\n", (long long)k); std::exit(2); }
                    out.entries.push_back(WalkEntry{ordinal, vx.raw, 0, vx.value});
                    at += 1;
                });
                if (k == c) out.end_pos = c * P + end;
                else if (end >= 0) { std::fprintf(stderr, "a chunk before the last reports the end\n"); std::exit(2); }
            }
            out.end_state = jr_jump(s0, (uint64_t)out.end_pos);
            return out;
        }
        if (fail_at[c]) { out.fail = true; return out; }
    }
    return out;
}

int64_t isqrt(int64_t v)
{
    int64_t r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

int64_t sphere_voxels(int64_t R)
{
    int64_t n = 0;
    for (int64_t dz = -R; dz <= R; ++dz) {
        const int64_t r1 = isqrt(R * R - dz * dz);
        for (int64_t dy = -r1; dy <= r1; ++dy) n += 2 * isqrt(r1 * r1 - dy * dy) + 1;
    }
    return n;
}

int cases = 0;

bool same(const Serial& s, const Chunked& c, const char* what, uint64_t s0, int64_t n, int P)
{
    bool ok = c.reached && !c.fail && c.end_state == s.end_state && c.end_pos == s.steps && c.entries.size() == s.items.size();
    for (size_t i = 0; ok && i < s.items.size(); ++i)
        ok = c.entries[i].ordinal == s.items[i].ordinal && c.entries[i].raw == s.items[i].raw && c.entries[i].value == s.items[i].value;
    if (!ok)
        std::fprintf(stderr, "MISMATCH %s: state %llx, n %lld, chunk %d: reached %d fail %d, end %lld / %ld, entries %zu / %zu\n", what,
                     (unsigned long long)s0, (long long)n, P, (int)c.reached, (int)c.fail, (long long)c.end_pos, s.steps, c.entries.size(),
                     s.items.size());
    cases += 1;
    return ok;
}

uint64_t scramble(uint64_t seed) { return (seed ^ MUL) & MASK; }

uint64_t inverse_multiplier()
{
    uint64_t x = MUL;                                   // Newton: x <- x (2 - a x), correct bits double each round
    for (int i = 0; i < 6; ++i) x = (x * (2 - MUL * x)) & MASK;
    return x;
}

}  // namespace

int main()
{
    bool ok = true;
    const int chunks[3] = {512, 513, SW_CHUNK};
    const int64_t radii[3] = {0, 1, 16};
    if (sphere_voxels(0) != 1 || sphere_voxels(1) != 7 || sphere_voxels(16) > 15700) { std::fprintf(stderr, "sphere sizes\n"); return 1; }

    // seeds 1..8, both rules, bounds 10 and 20, three radii, three chunk sizes
    for (int kind = 0; kind < 2; ++kind)
        for (int scale = 1; scale <= 2; ++scale)
            for (uint64_t seed = 1; seed <= 8; ++seed)
                for (int64_t R : radii) {
                    const int64_t n = sphere_voxels(R);
                    const uint64_t s0 = scramble(seed);
                    const Serial s = serial_walk(s0, n, kind, scale);
                    const WalkRule rule{10 * scale, kind, (int64_t)(7 * scale) * (7 * scale) * (7 * scale)};
                    for (int P : chunks)
                        ok = same(s, chunked_walk(s0, n, rule, P, SW_ENTRIES, P == SW_CHUNK ? SW_MAX_EVENTS : 4095, P == 513 ? 7 : 3), "seeds", s0, n, P) && ok;
                }

    // crafted states: voxel m retries nextInt once -- the state after 3 m + 1 steps is ((2^31 - 1) << 17) | low
    const uint64_t inv = inverse_multiplier();
    if (((inv * MUL) & MASK) != 1) { std::fprintf(stderr, "inverse multiplier\n"); return 1; }
    const int64_t n16 = sphere_voxels(16);
    for (int kind = 0; kind < 2; ++kind)
        for (int scale = 1; scale <= 2; ++scale)
            for (int P : chunks) {
                const int64_t ms[5] = {0, 1, P / 3 - 1, P / 3, P / 3 + 1};
                for (int64_t m : ms) {
                    bool found = false;
                    for (uint64_t low = 0; low < (1u << 17) && !found; ++low) {
                        uint64_t s0 = (((1ULL << 31) - 1) << 17) | low;
                        for (int64_t k = 0; k < 3 * m + 1; ++k) s0 = ((s0 - ADD) * inv) & MASK;
                        const Serial head = serial_walk(s0, m + 1, kind, scale);
                        bool plain = true;
                        for (int64_t i = 0; i < m; ++i) plain = plain && head.f[(size_t)i] == 3;
                        if (!plain) continue;
                        found = true;
                        if (head.f[(size_t)m] != 4 && head.f[(size_t)m] != 6) { std::fprintf(stderr, "voxel %lld does not retry (f = %d)\n", (long long)m, head.f[(size_t)m]); ok = false; }
                        const Serial s = serial_walk(s0, n16, kind, scale);
                        const WalkRule rule{10 * scale, kind, (int64_t)(7 * scale) * (7 * scale) * (7 * scale)};
                        ok = same(s, chunked_walk(s0, n16, rule, P, SW_ENTRIES, P == SW_CHUNK ? SW_MAX_EVENTS : 4095, 5), "retry", s0, n16, P) && ok;
                        ok = same(serial_walk(s0, m + 1, kind, scale), chunked_walk(s0, m + 1, rule, P, SW_ENTRIES, 4095, 5), "retry, last voxel", s0, m + 1, P) && ok;
                    }
                    if (!found) { std::fprintf(stderr, "no retry state for m = %lld, chunk %d\n", (long long)m, P); ok = false; }
                }
            }

    // the fallback report: one entry offset (every orbit that does not enter a chunk at 0 is out of range), or an event list of one entry
    {
        const uint64_t s0 = scramble(3);
        const WalkRule draw{10, SW_RULE_DRAW, 343};
        const Chunked few_entries = chunked_walk(s0, n16, draw, 512, 1, 4095, 3);
        if (!few_entries.fail || !few_entries.entries.empty()) { std::fprintf(stderr, "E = 1 did not raise the exceeded flag\n"); ok = false; }
        const Chunked few_events = chunked_walk(s0, n16, draw, 512, SW_ENTRIES, 1, 3);
        if (!few_events.fail || !few_events.entries.empty()) { std::fprintf(stderr, "a full event list did not raise the flag\n"); ok = false; }
        cases += 2;
    }
    if (!ok) return 1;
    std::fprintf(stderr, "sphere walk ok: %d cases\n", cases);
    return 0;
}
