// group_reduce.h — NumPy's add.reduce of one long run by a whole workgroup, in NumPy's bits (fiducials.hip).
//
// segment_stats.h states the sum (an accumulator that takes the pairwise sum of each 8192-element chunk in order) and
// walks it with one lane; that suits many short runs.  A fiducial is tens of runs of 10^4 .. 10^5 terms, so here one
// workgroup of WAVES waves takes one run:
//
//   full chunk     8192 terms are a balanced tree over 64 blocks of 128 (every split of 8192, 4096, .. 256 is a multiple
//                  of 8, so NumPy halves exactly).  Lane l of a wave sums block l with segstats::block_sum (the eight
//                  strided accumulators and their combine order), then six xor-butterfly steps add neighbours 1, 2, 4,
//                  .. 32 apart: at step d lane l holds the sum of the 2d blocks around it, left + right or right + left,
//                  which IEEE addition does not tell apart.  Every lane ends with the chunk's sum.  The waves take
//                  WAVES chunks at a time and the chunk sums enter the accumulator in chunk order.
//   last chunk     fewer than 8192 terms split at n / 2 rounded down to a multiple of 8, which is not lane-regular.  One
//                  lane walks the recursion twice: first to list its leaves (at most 128 terms each; a node above 128
//                  has halves of at least 64, so there are fewer than 128 leaves), then, after the lanes have summed one
//                  leaf each, to add the leaf sums in the recursion's order.
//
// term(p) is called exactly once for every p of [a, b), from some lane.  No contraction.
#pragma once
#include "segment_stats.h"

#pragma clang fp contract(off)

namespace pmi {
namespace groupreduce {

constexpr int WAVES = 4;                 // the workgroup is WAVES * 64 lanes
constexpr int MAX_LEAVES = 128;

template <typename S>
struct Shared {
    S chunk[WAVES];
    S leaf[MAX_LEAVES];
    int32_t leaf_lo[MAX_LEAVES], leaf_m[MAX_LEAVES];
    int32_t n_leaves;
};

// segstats::pairwise_sum with the 128-term blocks left to the caller: leaf(lo, m) gives the sum of one
template <typename S, typename Leaf>
__device__ inline S pairwise_walk(Leaf leaf, int32_t lo, int32_t m)
{
    constexpr int DEPTH = segstats::DEPTH;
    int32_t f_lo[DEPTH], f_m[DEPTH];
    S f_left[DEPTH];
    int f_state[DEPTH];
    f_lo[0] = lo, f_m[0] = m, f_state[0] = 0, f_left[0] = 0;
    int sp = 1;
    S ret = 0;
    // every frame is visited three times and there are fewer than m / 32 + 2 of them
    for (int32_t it = 0; it < 3 * (m / 32 + 2) && sp > 0; ++it) {
        const int t = sp - 1;
        const int32_t cm = f_m[t], clo = f_lo[t];
        int32_t half = cm / 2;
        half -= half % 8;
        if (f_state[t] == 0) {
            if (cm <= 128 || sp == DEPTH) {          // sp == DEPTH cannot happen within a chunk
                ret = leaf(clo, cm);
                --sp;
            } else {
                f_state[t] = 1;
                f_lo[sp] = clo, f_m[sp] = half, f_state[sp] = 0, f_left[sp] = 0;
                ++sp;
            }
        } else if (f_state[t] == 1) {
            f_left[t] = ret;
            f_state[t] = 2;
            f_lo[sp] = clo + half, f_m[sp] = cm - half, f_state[sp] = 0, f_left[sp] = 0;
            ++sp;
        } else {
            ret = f_left[t] + ret;
            --sp;
        }
    }
    return ret;
}

// NumPy's add.reduce of term(p), p in [a, b), 0 <= a <= b < 2^31.  Every lane of the WAVES * 64 lane workgroup calls it
// with the same a, b and sh, and every lane gets the sum.
template <typename S, typename F>
__device__ inline S reduce_sum(F term, int32_t a, int32_t b, Shared<S> &sh)
{
    constexpr int32_t CHUNK = segstats::CHUNK;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int32_t full = (b - a) / CHUNK;
    S acc = 0;
    for (int32_t c0 = 0; c0 < full; c0 += WAVES) {
        const int32_t c = c0 + wave;
        if (c < full) {                                              // the same for a whole wave
            S v = segstats::block_sum<S>(term, a + c * CHUNK + lane * 128, 128);
            for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
            if (lane == 0) sh.chunk[wave] = v;
        }
        __syncthreads();
        for (int w = 0; w < WAVES && c0 + w < full; ++w) acc += sh.chunk[w];
        __syncthreads();
    }
    const int32_t lo = a + full * CHUNK, m = b - lo;
    if (m > 0) {
        if (threadIdx.x == 0) {
            int32_t n = 0;
            pairwise_walk<S>([&](int32_t l, int32_t k) {
                if (n < MAX_LEAVES) sh.leaf_lo[n] = l, sh.leaf_m[n] = k;
                ++n;
                return (S)0;
            }, lo, m);
            sh.n_leaves = n;
        }
        __syncthreads();
        const int32_t n = sh.n_leaves;
        if (n <= MAX_LEAVES) {
            if ((int32_t)threadIdx.x < n) sh.leaf[threadIdx.x] = segstats::block_sum<S>(term, sh.leaf_lo[threadIdx.x], sh.leaf_m[threadIdx.x]);
            __syncthreads();
            if (threadIdx.x == 0) {
                int32_t at = 0;
                sh.chunk[0] = pairwise_walk<S>([&](int32_t, int32_t) { return sh.leaf[at++]; }, lo, m);
            }
        } else if (threadIdx.x == 0) {                               // more leaves than the list holds: cannot happen below 8192 terms
            sh.chunk[0] = segstats::pairwise_sum<S>(term, lo, m);
        }
        __syncthreads();
        acc += sh.chunk[0];
        __syncthreads();
    }
    return acc;
}

}  // namespace groupreduce
}  // namespace pmi
