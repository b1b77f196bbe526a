// The round schedule of the role-split fused rotate kernel (rotate_fft.hip: k_rotate_attenuate_fftx_roles).
//
// A block walks a geometry chunk in batches of ROT_ROUND_ROWS rows.  A batch whose rows all lie outside the volume
// (class 0) is a run of zero rows and takes no round; every other batch (class 1: all taps inside, class 2: mixed) is
// one round: the walker waves fill a round buffer, every wave of the block meets at ONE barrier, the transformer waves
// turn the buffer into spectrum rows while the walkers fill the other buffer.  Both roles iterate THIS enumeration and
// nothing else decides when a barrier is reached: it depends on block-uniform data only (the chunk's row count, the
// per-batch class table, the buffer the previous chunk left off at), so the two roles cannot disagree about the number
// of barriers.  Host code (tests/c_abi/rotate_rounds_main.cpp) checks the schedule's properties on the CPU.
#pragma once

#if defined(__HIPCC__)
#define MVSIM_RR_FN __host__ __device__
#else
#define MVSIM_RR_FN
#endif

namespace mvsim {
namespace fft {

constexpr int ROT_ROUND_ROWS = 8;    // rows per batch (the fused kernels' U)
constexpr int ROT_ROUND_BUFS = 2;    // round buffers: round r takes buffer r % 2 of the plane's running round count

struct RotRounds {
    int cnt;    // rows of the chunk
    int r0;     // first row (chunk-relative) of the batch rot_rounds_next returns next
    int buf;    // buffer of the next round; carried from chunk to chunk
};

struct RotBatch {
    int r0;      // first row of the batch, chunk-relative: rows r0 .. r0 + nrows - 1
    int nrows;   // 1 .. ROT_ROUND_ROWS (less than ROT_ROUND_ROWS only in a chunk's last batch)
    int cls;     // the class table's entry: 0 = zero rows, no round, no barrier; 1, 2 = one round
    int buf;     // the round's buffer; -1 for class 0
};

MVSIM_RR_FN inline RotRounds rot_rounds_begin(int cnt, int buf)
{
    return RotRounds{cnt, 0, buf};
}

// The next batch of the chunk; false once the chunk is exhausted (st.buf then is where the next chunk begins).
// `cls_of(b)` returns batch b's class; on the device it must return a block-uniform value.
template <class CLS>
MVSIM_RR_FN inline bool rot_rounds_next(RotRounds& st, const CLS& cls_of, RotBatch& b)
{
    if (st.r0 >= st.cnt) return false;
    b.r0 = st.r0;
    b.nrows = st.cnt - st.r0 < ROT_ROUND_ROWS ? st.cnt - st.r0 : ROT_ROUND_ROWS;
    b.cls = cls_of(st.r0 / ROT_ROUND_ROWS);
    if (b.cls == 0) {
        b.buf = -1;
    } else {
        b.buf = st.buf;
        st.buf = (st.buf + 1) % ROT_ROUND_BUFS;
    }
    st.r0 += ROT_ROUND_ROWS;
    return true;
}

// Which transformer (of nt) owns row u of a batch, and the rows of transformer t: contiguous groups of
// ROT_ROUND_ROWS / nt rows, so that a group is one multi-row call of the plan.
MVSIM_RR_FN constexpr int rot_round_group(int nt) { return ROT_ROUND_ROWS / nt; }
MVSIM_RR_FN constexpr int rot_round_owner(int u, int nt) { return u / rot_round_group(nt); }

}  // namespace fft
}  // namespace mvsim
