// The PSF spectrum cache's policy (csrc/psf_cache.h) in a program of its own: plain g++ under ASan + UBSan, no HIP, no libmvsim.so.
// "Device" memory is malloc / free through the cache's two function pointers, counted here, so that a leak, a double free or a use of a
// freed buffer is the sanitizer's to find.  Covered:
//   * a hit needs the same key AND the same taps; one bit in one tap, another kdim, or any single key field is a miss;
//   * equal hashes of different contents are a miss (the hash replaced by a constant: every lookup then lives on the memcmp alone);
//   * least recently used goes first, a hit refreshes, an entry's own bytes decide how many leave;
//   * the byte cap holds after every insert; an entry larger than the cap is refused and evicts nothing;
//   * an evicted entry of the same sizes hands its buffers over (no allocation), other sizes are freed and allocated;
//   * an allocation that fails leaves the cache as it was, minus what had to leave; discard; clear keeps the counters and frees all.
// Prints "psf cache ok: <n> checks" on stderr; any failure returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "psf_cache.h"

using namespace mvsim;

static long checks = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        ++checks;                                                           \
        if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static std::set<void*> g_live;
static long g_allocs = 0, g_frees = 0;
static bool g_fail_alloc = false;
static void* dev_alloc(size_t bytes)
{
    if (g_fail_alloc) return nullptr;
    void* p = std::malloc(bytes ? bytes : 1);
    g_live.insert(p);
    ++g_allocs;
    return p;
}
static void dev_free(void* p)
{
    if (!g_live.erase(p)) { std::fprintf(stderr, "free of a pointer the cache does not own\n"); std::abort(); }
    std::free(p);
    ++g_frees;
}
static uint64_t same_hash(const void*, size_t, uint64_t) { return 42u; }

static PsfKey key_of(int kx, int ky, int kz)
{
    PsfKey k{};
    k.kdim[0] = kx; k.kdim[1] = ky; k.kdim[2] = kz;
    k.px = 144; k.py = 144; k.pyb = 144; k.hxp = 80; k.zdirect = 1; k.tile_y = 8; k.views = 1;
    return k;
}

static std::vector<float> taps_of(size_t n, unsigned seed)
{
    std::vector<float> t(n);
    unsigned s = seed * 2654435761u + 1u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; t[i] = (float)(s >> 8) / 16777216.0f; }
    return t;
}

static int content_and_key(PsfCache::Hash hash)
{
    PsfCache c;
    c.configure(dev_alloc, dev_free, hash);
    const size_t n = 7 * 7 * 5, g2 = 4096, cap = 1 << 20;
    const PsfKey k = key_of(7, 7, 5);
    std::vector<float> a = taps_of(n, 1);
    CHECK(c.find(k, a.data(), n) == nullptr);
    PsfCache::Entry* ea = c.insert(k, a.data(), n, g2, cap);
    CHECK(ea && !ea->filled && ea->g2 && ea->psf && ea->g2_bytes == g2 && ea->psf_bytes == n * sizeof(float));
    CHECK(ea->taps == a && ea->taps.data() != a.data());                        // its own copy
    ea->filled = true;
    std::vector<float> a2 = a;                                                    // equal contents at another address: a hit
    CHECK(c.find(k, a2.data(), n) == ea && c.stats().hits == 1 && c.stats().misses == 1);
    // one ulp in one tap, first, middle and last: a miss -- also when every hash is the same
    for (size_t at : {(size_t)0, n / 2, n - 1}) {
        std::vector<float> b = a;
        uint32_t u;
        std::memcpy(&u, &b[at], 4); u += 1u; std::memcpy(&b[at], &u, 4);
        CHECK(c.find(k, b.data(), n) == nullptr);
    }
    // every key field by itself
    for (int f = 0; f < 11; ++f) {
        PsfKey q = k;
        if (f < 3) { q.kdim[f] += 2; q.kdim[(f + 1) % 3] -= 2; }                   // (the same tap count: only the key tells them apart)
        int32_t* w[8] = {&q.px, &q.py, &q.pyb, &q.hxp, &q.zdirect, &q.tile_y, &q.views, &q.reserved};
        if (f >= 3) *w[f - 3] += 1;
        CHECK(c.find(q, a.data(), n) == nullptr);
    }
    // fewer taps that agree as far as they go
    CHECK(c.find(k, a.data(), n - 1) == nullptr);
    CHECK(c.stats().hits == 1 && c.entries() == 1);
    // a second PSF under the same key: both are held, each found by its own contents
    std::vector<float> b = taps_of(n, 2);
    PsfCache::Entry* eb = c.insert(k, b.data(), n, g2, cap);
    CHECK(eb && eb != ea && eb->g2 != ea->g2 && eb->psf != ea->psf);
    CHECK(c.find(k, a.data(), n) == ea && c.find(k, b.data(), n) == eb);
    CHECK(c.stats().bytes == (int64_t)(2 * (g2 + n * sizeof(float))));
    return 0;
}

static int lru_and_cap()
{
    PsfCache c;
    c.configure(dev_alloc, dev_free);
    const size_t n = 64, g2 = 1000, each = g2 + n * sizeof(float), cap = 3 * each + each / 2;     // three entries fit, four do not
    const PsfKey k = key_of(4, 4, 4);
    std::vector<std::vector<float>> t;
    for (unsigned i = 0; i < 6; ++i) t.push_back(taps_of(n, 10 + i));
    for (int i = 0; i < 3; ++i) CHECK(c.insert(k, t[(size_t)i].data(), n, g2, cap) != nullptr);
    CHECK(c.entries() == 3 && c.stats().evictions == 0 && c.stats().bytes == (int64_t)(3 * each));
    CHECK(c.find(k, t[0].data(), n) != nullptr);                                  // 0 is the most recent now: 1 is the oldest
    const long allocs = g_allocs, frees = g_frees;
    PsfCache::Entry* e3 = c.insert(k, t[3].data(), n, g2, cap);
    CHECK(e3 && c.stats().evictions == 1 && c.entries() == 3 && (size_t)c.stats().bytes <= cap);
    CHECK(g_allocs == allocs && g_frees == frees);                                // same sizes: the evicted entry's buffers, handed over
    CHECK(c.find(k, t[1].data(), n) == nullptr);                                  // 1 left
    CHECK(c.find(k, t[2].data(), n) && c.find(k, t[0].data(), n) && c.find(k, t[3].data(), n));
    // order now (oldest first): 2, 0, 3.  A larger entry -- two of the small ones must leave, their buffers are freed, new ones allocated
    const size_t g2_big = 2 * g2 + n * sizeof(float);
    PsfCache::Entry* big = c.insert(k, t[4].data(), n, g2_big, cap);
    CHECK(big && c.stats().evictions == 3 && c.entries() == 2 && (size_t)c.stats().bytes <= cap);
    CHECK(g_frees == frees + 4 && g_allocs == allocs + 2);
    CHECK(c.find(k, t[2].data(), n) == nullptr && c.find(k, t[0].data(), n) == nullptr && c.find(k, t[3].data(), n) != nullptr);
    // an entry that alone exceeds the cap is refused and evicts nothing; it is a miss all the same
    const int64_t misses = c.stats().misses;
    CHECK(c.insert(k, t[5].data(), n, cap, cap) == nullptr);
    CHECK(c.entries() == 2 && c.stats().evictions == 3 && c.stats().misses == misses + 1);
    // a cap of 0: nothing is held
    CHECK(c.insert(k, t[5].data(), n, g2, 0) == nullptr && c.entries() == 2);
    // no device memory: nothing is added, nothing leaks
    g_fail_alloc = true;
    const size_t live = g_live.size();
    CHECK(c.insert(k, t[5].data(), n, 10, cap) == nullptr);
    g_fail_alloc = false;
    CHECK(g_live.size() <= live && c.find(k, t[5].data(), n) == nullptr);
    // discard: the entry is gone, its bytes too
    const int64_t held = c.stats().bytes;
    PsfCache::Entry* d = c.insert(k, t[5].data(), n, 10, cap);
    CHECK(d != nullptr);
    c.discard(d);
    CHECK(c.stats().bytes == held && c.find(k, t[5].data(), n) == nullptr);
    // release: no bytes, no entries, no device memory; the counters stay, and the next lookup misses
    const PsfCache::Stats before = c.stats();
    c.clear();
    CHECK(c.entries() == 0 && c.stats().bytes == 0 && g_live.empty());
    CHECK(c.stats().hits == before.hits && c.stats().misses == before.misses && c.stats().evictions == before.evictions);
    CHECK(c.find(k, t[3].data(), n) == nullptr);
    CHECK(c.insert(k, t[3].data(), n, g2, cap) != nullptr && c.stats().bytes == (int64_t)each);
    return 0;                                                                     // (the destructor frees the last entry)
}

// A, B, A, B under a cap that holds one entry: four misses, three evictions, one pair of buffers for all four
static int thrash()
{
    PsfCache c;
    c.configure(dev_alloc, dev_free);
    const size_t n = 125, g2 = 5000, cap = g2 + n * sizeof(float) + 100;
    const PsfKey k = key_of(5, 5, 5);
    const std::vector<float> a = taps_of(n, 3), b = taps_of(n, 4);
    const long allocs = g_allocs;
    for (int i = 0; i < 4; ++i) {
        const std::vector<float>& t = i % 2 ? b : a;
        CHECK(c.find(k, t.data(), n) == nullptr);
        PsfCache::Entry* e = c.insert(k, t.data(), n, g2, cap);
        CHECK(e && !e->filled && c.entries() == 1);
        e->filled = true;
    }
    CHECK(c.stats().misses == 4 && c.stats().hits == 0 && c.stats().evictions == 3 && g_allocs == allocs + 2);
    return 0;
}

int main()
{
    if (content_and_key(psf_hash64) || content_and_key(same_hash) || lru_and_cap() || thrash()) return 1;
    if (!g_live.empty() || g_allocs != g_frees) { std::fprintf(stderr, "device memory left: %zu blocks\n", g_live.size()); return 1; }
    // the hash itself: every length up to a few words, one flipped bit anywhere changes it
    std::vector<unsigned char> buf(100);
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = (unsigned char)(i * 37u + 11u);
    for (size_t len = 0; len <= buf.size(); ++len) {
        const uint64_t h = psf_hash64(buf.data(), len, 7);
        CHECK(h == psf_hash64(buf.data(), len, 7));
        CHECK(len == 0 || h != psf_hash64(buf.data(), len - 1, 7));
        for (size_t i = 0; i < len; ++i) {
            buf[i] ^= 0x10u;
            CHECK(psf_hash64(buf.data(), len, 7) != h);
            buf[i] ^= 0x10u;
        }
    }
    std::fprintf(stderr, "psf cache ok: %ld checks\n", checks);
    return 0;
}
