// The walk of drawSpheres (SimulateMultiViewDataset.java:436-522) and multiSpheres (SimulateMultiViewAberrations.java:474-586) over
// ONE sequential java.util.Random, stated so that it can be resolved in parallel.  Plain C++ under MVSIM_JR_FN, like jrandom.h: the
// kernels of sphere_walk.hip and tests/c_abi/sphere_walk_main.cpp compile the same statements.
//
// The generator state after p steps is jr_jump(s0, p) ("stream position p").  A voxel whose draws start at position p consumes f(p)
// steps: 1 for nextInt(bound), 1 more per retry of nextInt (the overflow test of the JDK, probability 3.7e-9 for bounds 10 and 20),
// 2 for nextDouble(), 2 more when that double is accepted -- and the next voxel starts at p + f(p).  f depends on the position alone,
// never on the voxel, so the start positions of the voxels are the orbit of 0 under p -> p + f(p).  Positions with f != 3 are EVENTS;
// between events the orbit advances by 3.  The stream is cut into chunks of P positions.  Per chunk and per entry offset e in
// [0, E) -- where the orbit enters the chunk -- walk_resolve() follows the orbit through the chunk's sorted event list and returns a
// WalkMap: the offset at which the orbit enters the next chunk, the voxels started and the voxels accepted on the way.  Maps compose
// (walk_compose), composition is associative, so a scan over the chunks gives every chunk its true entry, the ordinal of its first
// voxel and the index of its first accepted voxel; walk_chunk() then follows the true orbit once more and reports the accepted voxels.
// Whatever does not fit -- an orbit step that leaves [0, E), more events than a list holds -- raises `fail`: the caller walks on the
// host instead, the result is never silently wrong.
#pragma once

#include "jrandom.h"

namespace mvsim {

constexpr int SW_CHUNK = 4096;        // stream positions per chunk of the device walk
constexpr int SW_ENTRIES = 8;         // entry offsets resolved per chunk: steps of up to 8 (three retries of an accepted voxel)
constexpr int SW_MAX_EVENTS = 64;     // events a chunk's list holds (drawSpheres at scale 1, the densest: 12 expected)
constexpr int SW_MAX_CHUNK = 32768, SW_MAX_ENTRIES = 32, SW_CODE_STEPS = 127;   // what WalkMap::pack and an event word can hold

enum { SW_RULE_DRAW = 0, SW_RULE_MULTI = 1 };
struct WalkRule {
    int32_t bound;        // nextInt(bound): 10 * scale
    int32_t kind;         // SW_RULE_DRAW: Math.round(rv * 10000) % modulus == 0; SW_RULE_MULTI: rv * 100000 < 1
    int64_t modulus;      // (7 * scale)^3
};

struct WalkVoxel {
    int32_t steps;        // f(p)
    int32_t accepted;
    int32_t raw;          // what nextInt(bound) returned
    double  value;        // the second nextDouble() (accepted voxels only)
};

// what a walk reports per accepted voxel, in visit order
struct WalkEntry {
    int64_t ordinal;      // the voxel's place in the visit order of the large sphere
    int32_t raw, pad;
    double  value;
};

MVSIM_JR_FN bool walk_accepts(double rv, const WalkRule& r)
{
    if (r.kind == SW_RULE_MULTI) return rv * 100000 < 1;
    const int64_t rounded = (int64_t)floor(rv * 10000 + 0.5);     // Math.round; 0 .. 10000 as rv is in [0, 1)
    if (r.modulus > 10000) return rounded == 0;
    return (uint32_t)rounded % (uint32_t)r.modulus == 0;          // a 32-bit remainder: the 64-bit one is a subroutine on the GPU
}

// "if a voxel started at the position whose state is `state`": the serial statement, retries and all
MVSIM_JR_FN WalkVoxel walk_voxel(uint64_t state, const WalkRule& r)
{
    JRandom rnd{state};
    WalkVoxel v;
    v.steps = 1;
    int32_t x = rnd.next(31);                                      // JRandom::next_int with its steps counted
    const int32_t m = r.bound - 1;
    if ((r.bound & m) == 0) x = (int32_t)(((int64_t)r.bound * (int64_t)x) >> 31);
    else
        for (int32_t u = x; (int32_t)((uint32_t)u - (uint32_t)(x = u % r.bound) + (uint32_t)m) < 0; u = rnd.next(31)) v.steps += 1;
    v.raw = x;
    const double rv = rnd.next_double();
    v.steps += 2;
    v.accepted = walk_accepts(rv, r) ? 1 : 0;
    v.value = 0.0;
    if (v.accepted) {
        v.value = rnd.next_double();
        v.steps += 2;
    }
    return v;
}

// An event word: offset in the chunk | code << 16, code = steps | accepted << 7.  Steps beyond SW_CODE_STEPS do not fit: code 0xff.
MVSIM_JR_FN uint32_t walk_code_of(const WalkVoxel& v) { return v.steps > SW_CODE_STEPS ? 0xffu : (uint32_t)v.steps | ((uint32_t)v.accepted << 7); }
MVSIM_JR_FN uint32_t walk_event(int q, uint32_t code) { return (uint32_t)q | (code << 16); }
MVSIM_JR_FN int walk_event_q(uint32_t ev) { return (int)(ev & 0xffffu); }
MVSIM_JR_FN int walk_event_steps(uint32_t ev) { return (int)((ev >> 16) & 0x7fu); }
MVSIM_JR_FN int walk_event_accepted(uint32_t ev) { return (int)((ev >> 23) & 1u); }

// The code of the voxel that would start at the position whose state is w[0], from the six states w[0..5] a lane keeps in registers
// (w[i] = the state i steps on): one LCG step per position amortised.  A retry takes the serial statement.
MVSIM_JR_FN uint32_t walk_code(const uint64_t w[6], const WalkRule& r)
{
    const int32_t u = (int32_t)(w[1] >> 17), m = r.bound - 1;
    if ((r.bound & m) != 0 && (int32_t)((uint32_t)u - (uint32_t)(u % r.bound) + (uint32_t)m) < 0) return walk_code_of(walk_voxel(w[0], r));
    const int64_t hi = (int64_t)(w[2] >> 22) << 27;
    const double rv = (double)(hi + (int64_t)(w[3] >> 21)) * 0x1.0p-53;
    return walk_accepts(rv, r) ? (5u | 0x80u) : 3u;
}

struct WalkMap {
    int32_t exit;         // offset into the next chunk at which the orbit continues
    int32_t fail;
    int64_t count;        // voxels started in the chunk(s)
    int64_t accepted;     // ... of which accepted
    MVSIM_JR_FN uint32_t pack() const { return (uint32_t)exit | ((uint32_t)count << 5) | ((uint32_t)accepted << 19) | ((uint32_t)(fail ? 1 : 0) << 31); }
    static MVSIM_JR_FN WalkMap unpack(uint32_t w)
    {
        WalkMap m;
        m.exit = (int32_t)(w & 31u); m.count = (w >> 5) & 0x3fffu; m.accepted = (w >> 19) & 0xfffu; m.fail = (int32_t)(w >> 31);
        return m;
    }
};

// The orbit that enters a chunk of P positions at offset e, through the chunk's nev sorted events.  An event at q is on the orbit if
// and only if q >= p and (q - p) % 3 == 0; it contributes (q - p) / 3 + 1 voxels and moves the orbit to q + steps.
MVSIM_JR_FN WalkMap walk_resolve(const uint32_t* ev, int nev, int P, int e, int E, bool chunk_fail)
{
    WalkMap m;
    m.fail = chunk_fail ? 1 : 0;
    m.count = 0; m.accepted = 0;
    int p = e;
    for (int i = 0; i < nev; ++i) {
        const int q = walk_event_q(ev[i]);
        if (q < p || (q - p) % 3 != 0) continue;
        if (((ev[i] >> 16) & 0xffu) == 0xffu) m.fail = 1;
        m.count += (q - p) / 3 + 1;
        m.accepted += walk_event_accepted(ev[i]);
        p = q + walk_event_steps(ev[i]);
    }
    if (p < P) {
        const int n = (P - 1 - p) / 3 + 1;
        m.count += n;
        p += 3 * n;
    }
    m.exit = p - P;
    if (m.exit >= E) { m.fail = 1; m.exit = 0; }
    return m;
}

// first `a`, then the map `b` of the following chunk(s) at a's exit
MVSIM_JR_FN WalkMap walk_compose(const WalkMap& a, const WalkMap& b)
{
    WalkMap m;
    m.exit = b.exit; m.fail = a.fail | b.fail; m.count = a.count + b.count; m.accepted = a.accepted + b.accepted;
    return m;
}

// The true orbit through one chunk: entry offset e, `ordinal` = the ordinal of the voxel that starts there, at most n_total voxels in
// all.  emit(ordinal, q) for every accepted voxel with ordinal < n_total, in visit order.  Returns the voxels started here (capped at
// n_total - ordinal); *end = the offset, relative to the chunk, at which voxel n_total would start, when that is decided in this chunk
// (that is: when the chunk starts the last voxel), else -1.
template <class Emit>
MVSIM_JR_FN int64_t walk_chunk(const uint32_t* ev, int nev, int P, int e, int64_t ordinal, int64_t n_total, int64_t* end, Emit&& emit)
{
    const int64_t first = ordinal;
    int p = e;
    *end = -1;
    if (ordinal >= n_total) return 0;
    for (int i = 0; i < nev; ++i) {
        const int q = walk_event_q(ev[i]);
        if (q < p || (q - p) % 3 != 0) continue;
        const int64_t k = (q - p) / 3;
        if (ordinal + k >= n_total) {                              // the last voxel is a plain one in front of this event
            *end = p + 3 * (n_total - ordinal);
            return n_total - first;
        }
        if (walk_event_accepted(ev[i])) emit(ordinal + k, q);
        ordinal += k + 1;
        p = q + walk_event_steps(ev[i]);
        if (ordinal == n_total) {
            *end = p;
            return n_total - first;
        }
    }
    if (p < P) {
        const int64_t n = (P - 1 - p) / 3 + 1;
        if (ordinal + n >= n_total) {
            *end = p + 3 * (n_total - ordinal);
            return n_total - first;
        }
        ordinal += n;
    }
    return ordinal - first;
}

// Stream positions the device walk covers for n voxels.  5 n is the bound without retries; 3 n + n / 16 + 2 * SW_CHUNK is at least
// that for n <= SW_CHUNK and beyond leaves room for ten times the accepted voxels of the densest rule (3 in 1000) -- where it should not
// be enough the walk reports "not reached" and the caller walks on the host.
MVSIM_JR_FN int64_t walk_cover(int64_t n) { return 3 * n + n / 16 + 2 * SW_CHUNK; }

}  // namespace mvsim
