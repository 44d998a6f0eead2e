// rows_blocks.h — what the kernels over a table in block order share, on top of rows_common.h (pairs.hip, which makes
// the order; picks.hip and similar.hip, which read it).  A row's key is y_index << 32 | x_index and the rows are sorted
// by it; there is no K x L table of block starts: the rows of a run of blocks are two bisections of the sorted keys.
// Only the positions < p are visible: the reference's block table stops filling at the first sorted row whose index
// lies outside the K x L grid.  Each module's argument rules and messages stay in its own source (pairs accepts
// K > INDEX_MAX and tests it in the kernel, picks and similar refuse it).
#pragma once
#include <algorithm>

#include "rows_common.h"

namespace pmi {
namespace rows {

constexpr int64_t INDEX_MAX = 0xffffffffLL;      // no index reaches past 2^32

// the sorted keys, the row count, the visible prefix and the grid
struct Blocks {
    const uint64_t *keys;
    int32_t n, p;
    int64_t K, L;
};

__device__ __forceinline__ uint64_t block_key(int64_t k, int64_t l) { return ((uint64_t)k << 32) | (uint64_t)l; }

// visible rows of the blocks (k, l0 .. l1), all inside the grid: positions [a, b)
__device__ __forceinline__ void block_run(const Blocks &g, int64_t k, int64_t l0, int64_t l1, int32_t *a, int32_t *b)
{
    *a = lower_bound(g.keys, 0, g.p, block_key(k, l0));
    *b = lower_bound(g.keys, *a, g.p, block_key(k, l1) + 1u);
}

// The 3 x 3 blocks around (ki, li), clamped to the grid: the block columns l0 .. l1 (none when l0 > l1), and for
// t = 0 .. 2 whether block row ki - 1 + t holds one of them.  An index beyond [-1, K] x [-1, L] has no block of the
// nine inside, and no neighbour of it is computed.
struct Window {
    int64_t l0, l1;
    bool row[3];
};

__device__ __forceinline__ Window window(const Blocks &g, int64_t ki, int64_t li)
{
    Window w;
    w.l0 = li > 0 ? li - 1 : 0;
    w.l1 = std::min(li < g.L - 1 ? li + 1 : g.L - 1, INDEX_MAX);
    const bool near = ki >= -1 && ki <= g.K && li >= -1 && li <= g.L && w.l0 <= w.l1;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int64_t k = near ? ki - 1 + t : -1;
        w.row[t] = k >= 0 && k < g.K && k <= INDEX_MAX;
    }
    return w;
}

}  // namespace rows
}  // namespace pmi
