// Stand-alone check of the library's host-only headers (no HIP, no libmvsim.so): csrc/host_pool.h -- the host thread pool and the
// uint16 -> float32 widening of the 16-bit acquisition transfer -- and csrc/jrandom.h -- java.util.Random -- against the JDK's known
// answers, which tests/test_host_logic.py passes on the command line:
//   host_pool_main SEED RANDOM0_NEXTINT BOUND D <nextDouble ...> I <nextInt(BOUND) ...>
// Built with -fsanitize=address,undefined and with -fsanitize=thread.
#include "host_pool.h"
#include "jrandom.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace mvsim;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

static unsigned short value_at(long long i)
{
    const unsigned short edge[3] = {0, 1, 65535};
    return i < 3 ? edge[i] : (unsigned short)((i * 7 + 3) & 0xFFFF);      // a ramp that wraps through every 16-bit value
}

// n values into a destination `misalign` floats behind a 16-byte boundary; the floats around it must stay as they were
static void widen_case(long long n, int misalign, int threads)
{
    std::vector<unsigned short> src((size_t)n + 8);
    for (long long i = 0; i < (long long)src.size(); ++i) src[(size_t)i] = value_at(i);
    const float guard = -123.0f;
    std::vector<float> store((size_t)n + 16, guard);
    float* base = store.data();
    while ((reinterpret_cast<uintptr_t>(base) & 15) != 0) ++base;          // at most three floats
    float* dst = base + 4 + misalign;
    widen_u16_chunked({WidenJob{src.data(), dst, n}}, threads);
    long long bad = 0;
    for (long long i = 0; i < n; ++i) bad += dst[i] != (float)src[(size_t)i];
    EXPECT(bad == 0, "n=%lld misalign=%d threads=%d: %lld values differ from the scalar loop", n, misalign, threads, bad);
    EXPECT(dst[-1] == guard && dst[n] == guard, "n=%lld misalign=%d threads=%d: wrote outside [0, n)", n, misalign, threads);
}

// two contexts on two host threads: their jobs queue up behind each other, each sees all of its chunks exactly once
static void two_callers()
{
    auto caller = [](int id, int chunks, int threads, std::vector<int>* hits) {
        hits->assign((size_t)chunks, 0);
        for (int round = 0; round < 20; ++round)
            HostPool::get().run(chunks, threads, [&](int c) { (*hits)[(size_t)c] += id; });
    };
    std::vector<int> a, b;
    std::thread ta(caller, 1, 37, 3, &a), tb(caller, 2, 5, 16, &b);        // (5 chunks on 16 threads: more threads than chunks)
    ta.join(); tb.join();
    for (int h : a) EXPECT(h == 20, "caller 1: a chunk ran %d times in 20 rounds", h);
    for (int h : b) EXPECT(h == 40, "caller 2: a chunk ran %d times in 20 rounds", h / 2);
    int none = 0;
    HostPool::get().run(0, 4, [&](int) { ++none; });
    EXPECT(none == 0, "a job of no chunks ran something");
}

static void generator(int argc, char** argv)
{
    if (argc < 6) { EXPECT(false, "usage: host_pool_main SEED RANDOM0_NEXTINT BOUND D <doubles> I <ints>"); return; }
    const uint64_t seed = std::strtoull(argv[1], nullptr, 10);
    const long long first_int = std::atoll(argv[2]);
    const int bound = std::atoi(argv[3]);
    auto seeded = [](uint64_t s) { return JRandom{(s ^ JR_A) & JR_MASK}; };   // new Random(seed) scrambles the seed
    JRandom zero = seeded(0);
    EXPECT(zero.next(32) == first_int, "new Random(0).nextInt() = %d", zero.next(32));
    JRandom d = seeded(seed), k = seeded(seed);
    int nd = 0, ni = 0;
    char mode = 0;
    for (int i = 4; i < argc; ++i) {
        if (!std::strcmp(argv[i], "D") || !std::strcmp(argv[i], "I")) { mode = argv[i][0]; continue; }
        if (mode == 'D') { const double want = std::strtod(argv[i], nullptr), got = d.next_double(); EXPECT(got == want, "nextDouble %d: %a, JDK %a", nd, got, want); ++nd; }
        if (mode == 'I') { const int want = std::atoi(argv[i]), got = k.next_int(bound); EXPECT(got == want, "nextInt(%d) %d: %d, JDK %d", bound, ni, got, want); ++ni; }
    }
    EXPECT(nd >= 4 && ni >= 6, "only %d doubles and %d ints on the command line", nd, ni);
    // power-of-two bounds take the other branch of nextInt(bound): (bound * next(31)) >> 31
    JRandom p = seeded(seed), q = seeded(seed);
    EXPECT(p.next_int(16) == (int32_t)(((int64_t)16 * q.next(31)) >> 31), "nextInt(16)");
    // jump(s, k) = k single steps
    for (uint64_t steps : {0ULL, 1ULL, 2ULL, 63ULL, 64ULL, 1000003ULL}) {
        JRandom walk = seeded(seed);
        for (uint64_t i = 0; i < steps; ++i) (void)walk.next(32);
        EXPECT(jr_jump(seeded(seed).s, steps) == walk.s, "jump by %llu steps", (unsigned long long)steps);
    }
}

int main(int argc, char** argv)
{
    for (long long n : {0LL, 1LL, 7LL, 8LL, 9LL, (1LL << 20) - 1, 1LL << 20, (1LL << 20) + 3})
        for (int misalign : {0, 1})                                        // 16-byte aligned; only 4-byte aligned
            for (int threads : {1, 3, 16}) widen_case(n, misalign, threads);
    two_callers();
    generator(argc, argv);
    if (failures) return 1;
    std::printf("host pool and generator run ok\n");
    return 0;
}
