// csrc/rotate_rounds.h in a program of its own (plain g++, no HIP, no libmvsim.so): the round schedule of the role-split fused
// rotate kernel, walked the way the kernel's two roles walk it (rotate_fft.hip: k_rotate_attenuate_fftx_roles).
//   steps 1..40, 63, 64, 65, 511, 512; geometry chunks of 128 and 512 rows; 2 and 4 transformers; class tables all 0, all 1,
//   all 2, alternating and random (a chunk's partial last batch is class 2, as the kernel's classifier makes it).
// Checked: both roles see the same rounds in the same buffers and so execute the same number of barriers; every row of a
// batch that takes a round is transformed exactly once, every row of a class-0 batch gets exactly one zero store, no row
// outside the walk is touched; a round never takes the buffer of the round before it (whose readers may still be at work),
// and takes the buffer of the round two earlier, which its readers left before the barrier in between.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rotate_rounds.h"

using namespace mvsim::fft;

struct Round { int first_row, nrows, buf; };

static int fail(const char* what, int steps, int chunk, int nt, int table)
{
    std::fprintf(stderr, "rotate rounds: %s (steps %d, chunk %d, %d transformers, table %d)\n", what, steps, chunk, nt, table);
    return 1;
}

int main()
{
    std::vector<int> step_list;
    for (int s = 1; s <= 40; ++s) step_list.push_back(s);
    for (int s : {63, 64, 65, 511, 512}) step_list.push_back(s);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    long cases = 0;
    for (int steps : step_list)
        for (int chunk : {128, 512})
            for (int nt : {2, 4})
                for (int table = 0; table < 5; ++table) {
                    // the class of every batch of every chunk, as the kernel's classifier would leave it in LDS
                    std::vector<std::vector<int>> cls;
                    for (int c0 = 0; c0 < steps; c0 += chunk) {
                        const int cnt = steps - c0 < chunk ? steps - c0 : chunk;
                        std::vector<int> t((cnt + ROT_ROUND_ROWS - 1) / ROT_ROUND_ROWS);
                        for (size_t b = 0; b < t.size(); ++b) {
                            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                            t[b] = table < 3 ? table : (table == 3 ? (int)(b % 3) : (int)((rng >> 33) % 3));
                            if ((int)(b + 1) * ROT_ROUND_ROWS > cnt) t[b] = 2;
                        }
                        cls.push_back(t);
                    }
                    // the walkers' enumeration: one buffer fill and one barrier per round
                    std::vector<Round> walk;
                    {
                        int buf = 0, ci = 0;
                        for (int c0 = 0; c0 < steps; c0 += chunk, ++ci) {
                            const int cnt = steps - c0 < chunk ? steps - c0 : chunk;
                            RotRounds st = rot_rounds_begin(cnt, buf);
                            RotBatch b;
                            const std::vector<int>& t = cls[ci];
                            while (rot_rounds_next(st, [&](int i) { return t.at(i); }, b)) {
                                if (b.cls == 0) { if (b.buf != -1) return fail("class 0 with a buffer", steps, chunk, nt, table); continue; }
                                walk.push_back(Round{c0 + b.r0, b.nrows, b.buf});
                            }
                            buf = st.buf;
                        }
                    }
                    // every transformer's enumeration: its own state, its rows of every round, its share of the zero rows
                    std::vector<int> transformed(steps + ROT_ROUND_ROWS, 0), zeroed(steps + ROT_ROUND_ROWS, 0);
                    for (int tr = 0; tr < nt; ++tr) {
                        std::vector<Round> seen;
                        int buf = 0, ci = 0;
                        for (int c0 = 0; c0 < steps; c0 += chunk, ++ci) {
                            const int cnt = steps - c0 < chunk ? steps - c0 : chunk;
                            RotRounds st = rot_rounds_begin(cnt, buf);
                            RotBatch b;
                            const std::vector<int>& t = cls[ci];
                            while (rot_rounds_next(st, [&](int i) { return t.at(i); }, b)) {
                                if (b.cls == 0) {
                                    for (int j = tr; j < ROT_ROUND_ROWS; j += nt) zeroed.at(c0 + b.r0 + j) += 1;
                                    continue;
                                }
                                seen.push_back(Round{c0 + b.r0, b.nrows, b.buf});
                                const int rw = rot_round_group(nt);
                                for (int g = tr * rw; g < (tr + 1) * rw; ++g) {
                                    if (g >= b.nrows) break;
                                    if (rot_round_owner(g, nt) != tr) return fail("a row outside its owner's group", steps, chunk, nt, table);
                                    transformed.at(c0 + b.r0 + g) += 1;
                                }
                            }
                            buf = st.buf;
                        }
                        if (seen.size() != walk.size()) return fail("the roles disagree about the number of rounds", steps, chunk, nt, table);
                        for (size_t r = 0; r < seen.size(); ++r)
                            if (seen[r].buf != walk[r].buf || seen[r].first_row != walk[r].first_row || seen[r].nrows != walk[r].nrows)
                                return fail("the roles disagree about a round", steps, chunk, nt, table);
                    }
                    for (size_t r = 0; r < walk.size(); ++r) {
                        if (walk[r].buf < 0 || walk[r].buf >= ROT_ROUND_BUFS) return fail("no such buffer", steps, chunk, nt, table);
                        if (r >= 1 && walk[r].buf == walk[r - 1].buf) return fail("a buffer refilled while its round is being read", steps, chunk, nt, table);
                        if (r >= 2 && walk[r].buf != walk[r - 2].buf) return fail("a round not in the buffer two rounds back", steps, chunk, nt, table);
                    }
                    // rows: exactly one transform or exactly one zero store, by the class of the row's batch; nothing beyond the walk
                    {
                        int ci = 0;
                        for (int c0 = 0; c0 < steps; c0 += chunk, ++ci) {
                            const int cnt = steps - c0 < chunk ? steps - c0 : chunk;
                            for (int r = 0; r < cnt; ++r) {
                                const bool zero = cls[ci][r / ROT_ROUND_ROWS] == 0;
                                if (transformed[c0 + r] != (zero ? 0 : 1)) return fail("a row not transformed exactly once", steps, chunk, nt, table);
                                if (zeroed[c0 + r] != (zero ? 1 : 0)) return fail("a zero row not stored exactly once", steps, chunk, nt, table);
                            }
                        }
                        for (int r = steps; r < steps + ROT_ROUND_ROWS; ++r)
                            if (transformed[r] || zeroed[r]) return fail("a row beyond the walk", steps, chunk, nt, table);
                    }
                    cases += 1;
                }
    std::fprintf(stderr, "rotate rounds ok: %ld cases\n", cases);
    return 0;
}
