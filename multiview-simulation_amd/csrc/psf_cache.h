// PSF spectra cached by content (option psf_cache).  Plain C++: no HIP in here -- device memory comes from two function
// pointers, so that tests/c_abi/psf_cache_main.cpp runs the whole policy on the host under a sanitizer.
//
// An entry is what the convolution driver computes from a view's PSF alone: the compact spectrum G2 that psf_passes writes (a function of
// the NORMALISED taps and of the plan's geometry, nothing else), and the normalised taps on the device it was computed from.  The key is
// the geometry and the taps themselves: a 64-bit hash finds the candidates, and a candidate is accepted only after its key and ALL of its
// taps (the host copy the entry keeps) compare equal -- equal hashes of different PSFs are a miss.
// Replacement: least recently used under a cap on the device bytes held.  An evicted entry of the same sizes hands its buffers to the
// entry that replaces it (no free, no allocation); who may still be reading them is the caller's business (fft_driver.hip: psf_spectrum).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <list>
#include <vector>

namespace mvsim {

// Everything of a call that shapes G2, beside the taps.  No padding bytes: compared with memcmp.
struct PsfKey {
    int64_t kdim[3];
    int32_t px, py, pyb, hxp;       // ConvPlan: padded x and y lengths, rows of a plane in the z-blocked layout, complex row pitch
    int32_t zdirect, tile_y;        // the layout psf_passes writes for the direct z pass; lines per tile of the y pass
    int32_t views, reserved;        // stacked views V (always 1: stacked views do not use the cache)
};
static_assert(sizeof(PsfKey) == 3 * 8 + 8 * 4, "PsfKey must not have padding");

// 64 bits over whole 8-byte words in four independent lanes (a 31^3 PSF is 119 KB on the host path of every view: ~5 us), the tail bytewise
inline uint64_t psf_hash64(const void* data, size_t bytes, uint64_t seed)
{
    const unsigned char* p = static_cast<const unsigned char*>(data);
    const uint64_t m = 0x9E3779B97F4A7C15ull;
    uint64_t h[4] = {seed ^ 0x243F6A8885A308D3ull, seed ^ 0x13198A2E03707344ull, seed ^ 0xA4093822299F31D0ull, seed ^ 0x082EFA98EC4E6C89ull};
    size_t i = 0;
    for (; i + 32 <= bytes; i += 32) {
        uint64_t w[4];
        std::memcpy(w, p + i, 32);
        for (int k = 0; k < 4; ++k) { h[k] = (h[k] ^ w[k]) * m; h[k] ^= h[k] >> 29; }
    }
    uint64_t r = (uint64_t)bytes * m;
    for (; i < bytes; ++i) r = (r ^ p[i]) * 0x100000001B3ull;
    for (int k = 0; k < 4; ++k) { r = (r ^ h[k]) * m; r ^= r >> 32; }
    return r;
}

class PsfCache {
public:
    typedef void* (*DevAlloc)(size_t bytes);                 // null on failure
    typedef void (*DevFree)(void* p);
    typedef uint64_t (*Hash)(const void* data, size_t bytes, uint64_t seed);

    struct Entry {
        uint64_t hash = 0;
        PsfKey key{};
        std::vector<float> taps;        // the normalised PSF on the host: what a hit is compared against
        void* g2 = nullptr;             // device: G2 as psf_passes writes it
        void* psf = nullptr;            // device: the normalised PSF
        size_t g2_bytes = 0, psf_bytes = 0;
        bool filled = false;            // G2 has been enqueued (the driver sets it; an entry that is not filled is computed, not trusted)
    };
    struct Stats { int64_t hits = 0, misses = 0, evictions = 0, bytes = 0; };

    PsfCache() = default;
    PsfCache(const PsfCache&) = delete;
    PsfCache& operator=(const PsfCache&) = delete;
    ~PsfCache() { clear(); }

    void configure(DevAlloc a, DevFree f, Hash h = psf_hash64) { alloc_ = a; free_ = f; hash_ = h; }
    const Stats& stats() const { return stats_; }
    size_t entries() const { return lru_.size(); }

    // The entry of these taps under this key, most recently used from now on; null: not held.  Counts a hit.
    Entry* find(const PsfKey& key, const float* taps, size_t n)
    {
        const uint64_t h = hash_of(key, taps, n);
        for (auto it = lru_.begin(); it != lru_.end(); ++it) {
            if (it->hash != h || std::memcmp(&it->key, &key, sizeof(PsfKey)) != 0 || it->taps.size() != n) continue;
            if (std::memcmp(it->taps.data(), taps, n * sizeof(float)) != 0) continue;      // same hash, other PSF: a miss
            lru_.splice(lru_.begin(), lru_, it);
            stats_.hits += 1;
            return &lru_.front();
        }
        return nullptr;
    }

    // A new entry for taps that find() did not have: evicts from the least recently used end until the new entry fits under cap_bytes,
    // keeps a copy of the taps, and owns g2_bytes + n floats of device memory (not filled).  Counts a miss.  Null -- nothing held for
    // this PSF, the caller takes the uncached path -- when the entry alone exceeds the cap or the device has no memory for it.
    Entry* insert(const PsfKey& key, const float* taps, size_t n, size_t g2_bytes, size_t cap_bytes)
    {
        stats_.misses += 1;
        const size_t psf_bytes = n * sizeof(float), need = g2_bytes + psf_bytes;
        if (!alloc_ || !free_ || need > cap_bytes) return nullptr;
        void *g2 = nullptr, *psf = nullptr;
        while (!lru_.empty() && (size_t)stats_.bytes + need > cap_bytes) {
            Entry& v = lru_.back();
            if (!g2 && v.g2_bytes == g2_bytes && v.psf_bytes == psf_bytes) { g2 = v.g2; psf = v.psf; v.g2 = v.psf = nullptr; }
            drop_back();
            stats_.evictions += 1;
        }
        if (!g2) {
            g2 = alloc_(g2_bytes);
            psf = g2 ? alloc_(psf_bytes) : nullptr;
            if (!g2 || !psf) { if (g2) free_(g2); return nullptr; }
        }
        lru_.emplace_front();
        Entry& e = lru_.front();
        e.hash = hash_of(key, taps, n);
        e.key = key;
        e.taps.assign(taps, taps + n);
        e.g2 = g2; e.psf = psf; e.g2_bytes = g2_bytes; e.psf_bytes = psf_bytes;
        stats_.bytes += (int64_t)need;
        return &e;
    }

    // Forget an entry whose spectrum never came to be (a failed upload or launch).
    void discard(Entry* e)
    {
        for (auto it = lru_.begin(); it != lru_.end(); ++it)
            if (&*it == e) { lru_.splice(lru_.end(), lru_, it); drop_back(); return; }
    }

    // Every entry and its device memory; the counters of hits, misses and evictions stay.
    void clear()
    {
        while (!lru_.empty()) drop_back();
    }

private:
    uint64_t hash_of(const PsfKey& key, const float* taps, size_t n) const
    {
        return hash_(taps, n * sizeof(float), hash_(&key, sizeof(PsfKey), 0));
    }
    void drop_back()
    {
        Entry& v = lru_.back();
        if (v.g2) free_(v.g2);
        if (v.psf) free_(v.psf);
        stats_.bytes -= (int64_t)(v.g2_bytes + v.psf_bytes);
        lru_.pop_back();
    }

    std::list<Entry> lru_;              // front: most recently used
    Stats stats_;
    DevAlloc alloc_ = nullptr;
    DevFree free_ = nullptr;
    Hash hash_ = psf_hash64;
};

}  // namespace mvsim
