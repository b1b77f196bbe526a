// csrc/row_bits.h in a program of its own (plain g++, no HIP, no libmvsim.so): the row-bit record the fused rotate kernels write
// for pass B (rotate_fft.hip -> fft_passes.hip: k_fft_lines<PLAN, FWD, false>).
//   Ny in {1, 2, 5, 64, 77, 289, 512, 1024} x Ky in {1, 3, 9, 31, 63}, Py = the smallest length of the table >= Ny + Ky - 1 (what
//   custom_fft_sizes picks); stored-row sets: none, all, row 0 alone, row Ny - 1 alone, four random densities.
// Checked: the padded record equals a bit-by-bit restatement through map_src (fft_dev.h, copied below: mode 0 with pass B's zones,
// the general reflection included -- Ky = 63 on Ny = 1, 2, 5 has halos longer than the image); gap bits and the bits from Py on are
// clear; the device's form (64 positions per trip, two words) gives the same words; words per plane, bytes and alignment are what
// the driver allocates and the reader's scalar bursts assume.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "row_bits.h"

using namespace mvsim::fft;

// the length table (fft_dev.h: MVSIM_FFT_SIZES), lengths only
static const int kLens[] = {16, 18, 20, 24, 32, 36, 40, 48, 56, 64, 72, 80, 96, 112, 128, 140, 144, 160, 180, 192, 224, 256, 280, 288,
                            320, 350, 360, 384, 448, 512, 540, 560, 576, 640, 720, 768, 896, 1024, 1080, 1120, 1152, 1280, 1440, 1536,
                            1792, 2048, 2160, 2240};

static int pick_len(int need)
{
    for (int l : kLens)
        if (l >= need) return l;
    return -1;
}

// fft_dev.h: DimMap / map_src, mode 0 (mirror-single image padding)
struct DimMap { int n, P, a, b, mode, c; };
static int map_src(const DimMap& m, int j)
{
    int i;
    if (j < m.a) i = j;
    else if (j >= m.P - m.b) i = j - m.P;
    else return -1;
    if (i < 0) i = -i;
    if (i >= m.n) i = 2 * m.n - 2 - i;
    if (i >= 0 && i < m.n) return i;
    if (m.n == 1) return 0;
    const int p = 2 * m.n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < m.n ? i : p - i;
}

static int fail(const char* what, int ny, int ky, int py, int set)
{
    std::fprintf(stderr, "row bits: %s (Ny %d, Ky %d, Py %d, set %d)\n", what, ny, ky, py, set);
    return 1;
}

int main()
{
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    long cases = 0;
    for (int ny : {1, 2, 5, 64, 77, 289, 512, 1024})
        for (int ky : {1, 3, 9, 31, 63}) {
            const int py = pick_len(ny + ky - 1);
            if (py < 0) return fail("no length", ny, ky, py, -1);
            // sizes: what rotate_attenuate_fftx reserves (records behind a 256-byte boundary) and k_fft_lines loads
            const int words = row_bits_words(py);
            if (words * 32 < py) return fail("record shorter than the line", ny, ky, py, -1);
            if (words <= ROW_BITS_BURST ? (words & (words - 1)) != 0 : words % ROW_BITS_BURST != 0) return fail("not whole bursts", ny, ky, py, -1);
            const int align = row_bits_align(py);
            if (align != 4 * (words < ROW_BITS_BURST ? words : ROW_BITS_BURST) || 256 % align != 0) return fail("alignment", ny, ky, py, -1);
            for (int z : {0, 1, 7, 511})
                if (((size_t)z * words * sizeof(unsigned int)) % (size_t)align != 0) return fail("a record off its alignment", ny, ky, py, z);
            if (row_bits_bytes(py, 512) != (size_t)512 * words * 4) return fail("bytes", ny, ky, py, -1);
            if (row_bits_len_ok(py) != (words <= ROW_BITS_MAX_WORDS)) return fail("len_ok", ny, ky, py, -1);
            if (ny > 32 * ROW_BITS_MAX_WORDS && row_bits_len_ok(py)) return fail("data bits beyond the kernels' LDS words", ny, ky, py, -1);

            const DimMap lmap{ny, py, ny + ky / 2, ky - 1 - ky / 2, 0, 0};     // fft_driver.hip: pass_b
            for (int set = 0; set < 8; ++set) {
                std::vector<unsigned int> data((ny + 31) / 32 + 1, 0u);
                std::vector<char> stored(ny, 0);
                for (int y = 0; y < ny; ++y) {
                    bool s;
                    switch (set) {
                        case 0: s = false; break;
                        case 1: s = true; break;
                        case 2: s = y == 0; break;
                        case 3: s = y == ny - 1; break;
                        default: s = (int)(next() % 100) < (set == 4 ? 3 : set == 5 ? 50 : set == 6 ? 97 : 20); break;
                    }
                    stored[y] = s;
                    if (s) data[y >> 5] |= 1u << (y & 31);
                }
                std::vector<unsigned int> rec(words + 2, 0xDEADBEEFu);
                row_bits_expand(data.data(), rec.data(), ny, ky, py);
                if (rec[words] != 0xDEADBEEFu) return fail("wrote past the record", ny, ky, py, set);
                for (int n = 0; n < words * 32; ++n) {
                    const bool bit = (rec[n >> 5] >> (n & 31)) & 1u;
                    const int s = n < py ? map_src(lmap, n) : -1;
                    if (n < py && s != row_bits_src(n, ny, ky, py)) return fail("row_bits_src != map_src", ny, ky, py, n);
                    const bool want = s >= 0 && stored[s];
                    if (bit != want) return fail(s < 0 ? "a gap bit is set" : "bit != the source row's", ny, ky, py, n);
                    if (n < ny && bit != (bool)stored[n]) return fail("a data position does not carry its own bit", ny, ky, py, n);
                }
                // the device's form (rotate_dev.h: write_row_bits): a ballot over 64 positions, two words per trip
                for (int w0 = 0; w0 < words; w0 += 2) {
                    uint64_t m = 0;
                    for (int lane = 0; lane < 64; ++lane)
                        if (row_bits_padded_bit(data.data(), 32 * w0 + lane, ny, ky, py)) m |= (uint64_t)1 << lane;
                    for (int h = 0; h < 2; ++h)
                        if (w0 + h < words && rec[w0 + h] != (unsigned int)(m >> (32 * h))) return fail("ballot form differs", ny, ky, py, w0 + h);
                }
                cases += 1;
            }
        }
    std::fprintf(stderr, "row bits ok: %ld cases\n", cases);
    return 0;
}
