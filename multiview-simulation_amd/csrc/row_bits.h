// The row-bit record between the fused rotate kernels (rotate_fft.hip) and pass B (fft_passes.hip: k_fft_lines<PLAN, FWD, false>).
//
// A row of the attenuated plane without a non-zero voxel has the zero spectrum.  With the record in use the rotate kernel does not
// store such a row at all -- the workspace keeps whatever an earlier view left there -- and pass B does not read it: for plane z
// the record is a bit string over the PADDED y positions n in [0, Py) of pass B's line,
//     bit n set  <=>  position n reads a row the rotate kernel really stored (a transformed non-zero row).
// Data positions [0, Ny) carry their own row's bit, the two mirrored halos [Ny, Ny + Ky/2) and [Py - (Ky-1-Ky/2), Py) the bit of the
// row pass B's index map (map_src, mode 0) names there, the gap and everything from Py on 0: like the plane bit string of
// k_plane_flags_finish the reader gets ONE run of bits and maps no index of its own.  Rows the reference never visits (Ny > Nx)
// are zero rows.  Every block of the rotate kernel writes its plane's whole record on every launch, empty planes included.
// ANY reader of the rotate kernel's spectrum must ask these bits: an unflagged row holds stale bytes.
// Host code (tests/c_abi/row_bits_main.cpp) checks the expansion and the sizes on the CPU.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define MVSIM_RB_FN __host__ __device__
#else
#define MVSIM_RB_FN
#endif

namespace mvsim {
namespace fft {

constexpr int ROW_BITS_BURST = 16;       // words of the widest block-uniform (scalar) load
constexpr int ROW_BITS_MAX_WORDS = 48;   // records the kernels are built for: padded lines of up to 1536 points

// Words of a plane's record, a fixed function of Py: a power of two up to one burst, whole bursts beyond -- the record of plane z
// starts at word z * row_bits_words(Py) and is aligned to its own size (one burst) or to a burst
MVSIM_RB_FN constexpr int row_bits_words(int py)
{
    const int w = (py + 31) / 32;
    if (w <= ROW_BITS_BURST) {
        int p = 1;
        while (p < w) p *= 2;
        return p;
    }
    return (w + ROW_BITS_BURST - 1) / ROW_BITS_BURST * ROW_BITS_BURST;
}
// bytes the first word of every record is aligned to, given a base aligned at least that much
MVSIM_RB_FN constexpr int row_bits_align(int py)
{
    const int w = row_bits_words(py);
    return 4 * (w < ROW_BITS_BURST ? w : ROW_BITS_BURST);
}
MVSIM_RB_FN constexpr bool row_bits_len_ok(int py) { return py >= 1 && row_bits_words(py) <= ROW_BITS_MAX_WORDS; }
// what the driver allocates for `planes` records
MVSIM_RB_FN constexpr size_t row_bits_bytes(int py, int planes) { return (size_t)row_bits_words(py) * (size_t)planes * sizeof(unsigned int); }

// The row that padded position n of pass B's line reads (-1: the gap, or n outside [0, Py)): map_src of
// DimMap{ny, py, ny + ky / 2, ky - 1 - ky / 2, 0, 0} (fft_driver.hip: pass_b), restated here for the host
MVSIM_RB_FN inline int row_bits_src(int n, int ny, int ky, int py)
{
    const int a = ny + ky / 2, b = ky - 1 - ky / 2;
    if (n < 0 || n >= py) return -1;
    int i;
    if (n < a) i = n;
    else if (n >= py - b) i = n - py;
    else return -1;
    if (i < 0) i = -i;
    if (i >= ny) i = 2 * ny - 2 - i;
    if (i >= 0 && i < ny) return i;
    if (ny == 1) return 0;
    const int p = 2 * ny - 2;                 // a halo longer than the image
    i %= p;
    if (i < 0) i += p;
    return i < ny ? i : p - i;
}

// bit y of the Ny data bits `data` (words of 32 rows): row y was stored
MVSIM_RB_FN inline bool row_bits_data(const unsigned int* data, int y) { return (data[y >> 5] >> (y & 31)) & 1u; }

// bit n of the padded record
MVSIM_RB_FN inline bool row_bits_padded_bit(const unsigned int* data, int n, int ny, int ky, int py)
{
    const int s = row_bits_src(n, ny, ky, py);
    return s >= 0 && row_bits_data(data, s);
}

// the whole record of a plane from its data bits (the device does the same with one ballot per 64 positions)
MVSIM_RB_FN inline void row_bits_expand(const unsigned int* data, unsigned int* rec, int ny, int ky, int py)
{
    const int words = row_bits_words(py);
    for (int w = 0; w < words; ++w) {
        unsigned int v = 0u;
        for (int b = 0; b < 32; ++b)
            if (row_bits_padded_bit(data, 32 * w + b, ny, ky, py)) v |= 1u << b;
        rec[w] = v;
    }
}

}  // namespace fft
}  // namespace mvsim
