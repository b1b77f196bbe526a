// csrc/poisson_recipe.h in a program of its own (host compiler, -O2 -ffp-contract=off, no HIP, no libmvsim.so), linked with the
// oracle's C restatement (oracle/mvsim_oracle.c): the one statement of the sampler's per-voxel arithmetic against the oracle.
//   lambda : log-uniform over [1e-3, 1e15], rounded through float; every 64 tuples one each of exactly 10, the float below 10, 0, a
//            negative value and NaN
//   keys   : one with only a low word, one with both words, one all-ones
//   streams: 0, 1, 0x7fffffff, 0xffffffff, one per combination in turn
//   counters: 200 000 consecutive ones (mod 2^64) from 0, 2^32 - 100, 2^33 - 7, 2^63 - 50 and 2^64 - 300
// 15 combinations of key and counter range, 3 000 000 tuples.  On every tuple
//   * poisson_voxel equals orc_poisson_counter (as the float the kernels store);
//   * poisson_counter4 over every aligned group of four equals the same counts;
//   * the recipe WITHOUT the fp32 screen -- the attempt walk below: the same words, ptrs_fast, and ptrs_exact for every attempt the
//     squeeze leaves open -- gives the same count, and wherever ptrs_screen answers on such an attempt its answer is ptrs_exact's.
// The screen must have answered on a non-trivial share (> 1/4) of the exact tests it was shown below its lambda limit.
// Usage: poisson_recipe_main [noscreen]   -- `noscreen`: hold the screen-less walk alone to the oracle (the other checks are skipped)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mvsim_oracle.h"
#include "poisson_recipe.h"

using namespace mvsim;

static unsigned long long g_exact_seen = 0, g_screen_shown = 0, g_screen_answered = 0, g_screen_wrong = 0;

// One voxel by the recipe's pieces without the screen; tallies what the screen would have said.
static float voxel_without_screen(double lambda, uint32_t k0, uint32_t k1, uint32_t stream, uint64_t index)
{
    if (!(lambda > 0.0)) return 0.0f;
    if (lambda < 10.0) return poisson_small(lambda, group_word(group_block(index, stream, k0, k1), index));
    const PtrsSetup s = ptrs_setup(lambda);
    uint32_t w0, w1;
    pair_words(pair_block(index, stream, k0, k1), index, w0, w1);
    for (uint32_t att = 0u; att < kPtrsMaxAttempts; ++att) {
        if (att != 0u) ptrs_retry_words(index, att, k0, k1, stream, w0, w1);
        double us, V, kd;
        const int st = ptrs_fast(s, lambda, w0, w1, us, V, kd);
        if (st == 0) return count_as_float(kd);
        if (st == 1) continue;
        double loglam = 0.0;
        bool have = false;
        const bool accept = ptrs_exact(s, lambda, us, V, kd, loglam, have);
        const int sc = ptrs_screen(s, lambda, us, V, kd);
        g_exact_seen += 1;
        g_screen_shown += lambda < kScreenMaxLambda;
        g_screen_answered += sc != 0;
        g_screen_wrong += sc != 0 && (sc > 0) != accept;
        if (accept) return count_as_float(kd);
    }
    return (float)(long long)lambda;
}

int main(int argc, char** argv)
{
    const bool noscreen_only = argc > 1 && std::strcmp(argv[1], "noscreen") == 0;
    const uint64_t seeds[3] = {0x000000001BADB002ull, 0x9E3779B97F4A7C15ull, 0xFFFFFFFFFFFFFFFFull};
    const uint64_t starts[5] = {0ull, (1ull << 32) - 100ull, (1ull << 33) - 7ull, (1ull << 63) - 50ull, 0ull - 300ull};
    const uint32_t streams[4] = {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const int N = 200000;
    const double specials[5] = {10.0, (double)std::nextafterf(10.0f, 0.0f), 0.0, -3.5, std::numeric_limits<double>::quiet_NaN()};
    std::vector<double> lam((size_t)N);
    std::vector<float> want((size_t)N);
    uint64_t rng = 0x243F6A8885A308D3ull;
    unsigned long long tuples = 0, bad_voxel = 0, bad_four = 0, bad_noscreen = 0, small = 0, bright = 0;
    for (int si = 0; si < 3; ++si)
        for (int ci = 0; ci < 5; ++ci) {
            const uint32_t k0 = (uint32_t)seeds[si], k1 = (uint32_t)(seeds[si] >> 32);
            // the whole combination on one stream, so that its groups of four share their blocks as the kernels' do
            const uint32_t stream = streams[(si * 5 + ci) % 4];
            for (int t = 0; t < N; ++t) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                const double u = (double)(rng >> 11) * 0x1.0p-53;                          // [0, 1)
                lam[(size_t)t] = (double)(float)std::exp(std::log(1.0e-3) + u * (std::log(1.0e15) - std::log(1.0e-3)));
                if (t % 64 < 5) lam[(size_t)t] = specials[t % 64];
            }
            for (int t = 0; t < N; ++t) {
                const uint64_t index = starts[ci] + (uint64_t)t;                           // mod 2^64
                const double l = lam[(size_t)t];
                want[(size_t)t] = (float)orc_poisson_counter(l, seeds[si], stream, index);
                small += l > 0.0 && l < 10.0;
                bright += l >= 10.0;
                tuples += 1;
                if (voxel_without_screen(l, k0, k1, stream, index) != want[(size_t)t]) bad_noscreen += 1;
                if (noscreen_only) continue;
                if (poisson_voxel(l, k0, k1, stream, index) != want[(size_t)t]) {
                    if (bad_voxel++ < 10) std::fprintf(stderr, "poisson_voxel: lambda %.17g seed %d stream %u index %llu\n", l, si, stream, (unsigned long long)index);
                }
            }
            if (noscreen_only) continue;
            for (int t = (int)((4u - (unsigned)(starts[ci] & 3u)) & 3u); t + 4 <= N; t += 4) {
                float got[4];
                poisson_counter4(&lam[(size_t)t], k0, k1, stream, starts[ci] + (uint64_t)t, got);
                for (int c = 0; c < 4; ++c)
                    if (got[c] != want[(size_t)(t + c)]) {
                        if (bad_four++ < 10) std::fprintf(stderr, "poisson_counter4: lambda %.17g seed %d stream %u index %llu\n", lam[(size_t)(t + c)], si, stream,
                                                          (unsigned long long)(starts[ci] + (uint64_t)(t + c)));
                    }
            }
        }
    std::fprintf(stderr, "tuples %llu (inversion %llu, PTRS %llu); mismatches: poisson_voxel %llu, poisson_counter4 %llu, without the screen %llu\n", tuples,
                 small, bright, bad_voxel, bad_four, bad_noscreen);
    std::fprintf(stderr, "exact tests %llu, shown to the screen below its limit %llu, answered %llu, answered differently from the exact test %llu\n",
                 g_exact_seen, g_screen_shown, g_screen_answered, g_screen_wrong);
    if (bad_voxel || bad_four || bad_noscreen || g_screen_wrong) return 1;
    if (small < tuples / 20 || bright < tuples / 2) return 2;                              // the regimes were sampled
    if (4 * g_screen_answered < g_screen_shown || g_screen_shown < 1000) return 3;         // the screen did answer
    std::fprintf(stderr, "poisson recipe ok%s: %llu tuples\n", noscreen_only ? " (screen-less walk)" : "", tuples);
    return 0;
}
