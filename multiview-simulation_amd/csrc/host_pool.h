// Host side of the 16-bit acquisition transfer, and the host threads every bulk host loop of the library runs on.
// A 512^3 acquisition is 0.54 GB of float32 that hold small integers (Poisson counts, Tools.java:84): it crosses PCIe as 0.27 GB of
// uint16 and is widened here, by a few host threads with streaming stores (the destination -- the caller's buffer -- is written once
// and not read back by us), while the next view's transfer is already running.  Process-wide pool, created on first use.
// Plain C++ (no HIP): tests/c_abi/host_pool_main.cpp runs it under the address, undefined-behaviour and thread sanitizers.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include <emmintrin.h>

namespace mvsim {

class HostPool {
public:
    static HostPool& get() { static HostPool p; return p; }
    // fn(chunk) for chunk = 0 .. chunks-1 on up to `threads` threads (the caller's thread takes part); returns when all are done.
    // One job at a time: callers on different host threads (one context each) queue up behind each other.
    void run(int chunks, int threads, const std::function<void(int)>& fn)
    {
        if (chunks <= 0) return;
        std::lock_guard<std::mutex> one_job(run_m_);
        threads = std::max(1, std::min(threads, chunks));
        std::unique_lock<std::mutex> lk(m_);
        while ((int)workers_.size() < threads - 1) {
            const int id = (int)workers_.size();
            workers_.emplace_back([this, id] { loop(id); });
        }
        fn_ = &fn; next_ = 0; total_ = chunks; pending_ = chunks; helpers_ = threads - 1; gen_ += 1;
        cv_.notify_all();
        lk.unlock();
        work();
        lk.lock();
        done_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }
private:
    HostPool() = default;
    ~HostPool()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    void work()
    {
        for (;;) {
            int c;
            const std::function<void(int)>* f;
            {
                std::lock_guard<std::mutex> lk(m_);
                if (!fn_ || next_ >= total_) return;
                c = next_++; f = fn_;
            }
            (*f)(c);                                   // (run() does not return before pending_ is 0, so *f outlives every call)
            std::lock_guard<std::mutex> lk(m_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop(int id)
    {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || (gen_ != seen && fn_ && next_ < total_ && id < helpers_); });
                if (stop_) return;
                seen = gen_;
            }
            work();
        }
    }
    std::mutex m_, run_m_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> workers_;
    const std::function<void(int)>* fn_ = nullptr;
    int next_ = 0, total_ = 0, pending_ = 0, helpers_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
};

// dst[i] = (float) src[i], i in [0, n): 8 values per step, streaming stores where the destination is 16-byte aligned
inline void widen_u16(const unsigned short* src, float* dst, long long n)
{
    long long i = 0;
    while (i < n && (reinterpret_cast<uintptr_t>(dst + i) & 15) != 0) { dst[i] = (float)src[i]; ++i; }
    const __m128i zero = _mm_setzero_si128();
    for (; i + 8 <= n; i += 8) {
        const __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i));
        _mm_stream_ps(dst + i, _mm_cvtepi32_ps(_mm_unpacklo_epi16(v, zero)));
        _mm_stream_ps(dst + i + 4, _mm_cvtepi32_ps(_mm_unpackhi_epi16(v, zero)));
    }
    for (; i < n; ++i) dst[i] = (float)src[i];
    _mm_sfence();
}

// Several arrays widened as ONE job of the pool, in chunks of 1 Mi values (2 MB in, 4 MB out)
struct WidenJob {
    const unsigned short* src;
    float*                dst;
    long long             n;
};
inline void widen_u16_chunked(const std::vector<WidenJob>& arrays, int threads)
{
    const long long chunk = (long long)1 << 20;
    std::vector<WidenJob> jobs;
    for (const WidenJob& a : arrays)
        for (long long at = 0; at < a.n; at += chunk) jobs.push_back(WidenJob{a.src + at, a.dst + at, std::min(chunk, a.n - at)});
    HostPool::get().run((int)jobs.size(), threads, [&](int j) { widen_u16(jobs[(size_t)j].src, jobs[(size_t)j].dst, jobs[(size_t)j].n); });
}

}  // namespace mvsim
