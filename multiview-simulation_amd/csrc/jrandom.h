// java.util.Random (JDK specification): the 48-bit LCG the reference draws every phantom, bead and ray from.  One statement of the
// recipe for the host walks (phantom.hip, mvsim_beads_random_points) and the device tracers (aberrations.hip); plain C++, so the
// known answers of tests/golden/jdk_vectors.json check it without a GPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MVSIM_JR_FN __host__ __device__ __forceinline__
#else
#define MVSIM_JR_FN inline
#endif

namespace mvsim {

constexpr uint64_t JR_MASK = (1ULL << 48) - 1, JR_A = 0x5DEECE66DULL, JR_C = 0xBULL;

struct JRandom {
    uint64_t s;                       // the scrambled seed as the JDK keeps it (48 bits)
    MVSIM_JR_FN int32_t next(int bits)
    {
        s = (s * JR_A + JR_C) & JR_MASK;
        return (int32_t)((int64_t)s >> (48 - bits));
    }
    MVSIM_JR_FN int32_t next_int(int32_t bound)
    {
        int32_t r = next(31);
        const int32_t m = bound - 1;
        if ((bound & m) == 0) return (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
        for (int32_t u = r; (int32_t)((uint32_t)u - (uint32_t)(r = u % bound) + (uint32_t)m) < 0; u = next(31)) {}
        return r;
    }
    MVSIM_JR_FN double next_double()
    {
        const int64_t hi = (int64_t)next(26) << 27;
        return (double)(hi + next(27)) * 0x1.0p-53;
    }
};

// the state after k steps from s: s * a^k + c (a^(k-1) + ... + 1)  (mod 2^48), composing the affine map with itself by squaring
MVSIM_JR_FN uint64_t jr_jump(uint64_t s, uint64_t k)
{
    uint64_t A = 1, C = 0, a = JR_A, c = JR_C;
    while (k) {
        if (k & 1) { A = (A * a) & JR_MASK; C = (C * a + c) & JR_MASK; }
        c = ((a + 1) * c) & JR_MASK;
        a = (a * a) & JR_MASK;
        k >>= 1;
    }
    return (s * A + C) & JR_MASK;
}

}  // namespace mvsim
