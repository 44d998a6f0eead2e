// rows_groups.h — what the kernels over a table ordered by a label column share, on top of rows_common.h (centers.hip,
// kinetics.hip, combine.hip; areas.hip and average.hip read such a table): how a row index, a run and a sort key are
// made safe against an inconsistent table, the stable sort by "column - minimum", run closing, the gather of a column
// into the table's order and the dispatch over the column types.  Templates, as in rows_common.h: a source that does
// not use a piece carries none of it.
#pragma once
#include <type_traits>

#include "rows_common.h"

namespace pmi {
namespace rows {

__device__ __forceinline__ bool row_ok(int32_t i, int32_t n) { return (uint32_t)i < (uint32_t)n; }

// [a, b) of run g; an inconsistent start table gives an empty run, never a read out of bounds
__device__ __forceinline__ void run_of(const int32_t *__restrict__ start, int32_t g, int32_t n, int32_t *a, int32_t *b)
{
    *a = start[g];
    *b = start[g + 1];
    if (*a < 0 || *b > n || *a > *b) *a = *b = 0;
}

// Run closing, from inside a module's own start_kernel.  flag marks the first position of a run, pos is the exclusive
// scan of flag: run pos starts at a flagged p.  table[pos] = value there, and the last position closes the n + 1
// entries of the table with table[total] = end.  Returns pos + flag, the runs up to and including p: the total at
// p == n - 1.
__device__ __forceinline__ uint32_t close_runs(int64_t p, int32_t n, uint32_t flag, uint32_t pos, int32_t value,
                                               int32_t end, int32_t *__restrict__ table)
{
    const uint32_t total = pos + flag;
    if (flag && pos < (uint32_t)n) table[pos] = value;
    if (p == n - 1 && total <= (uint32_t)n) table[total] = end;
    return total;
}

// keys[p] = col[i] - lo as uint64 (a negative value comes first), i = rows ? rows[p] : p; the first key of a chain of
// sorts also writes the identity rows
template <typename T>
__global__ void column_key_kernel(const T *__restrict__ col, const int32_t *__restrict__ rows /* null: the identity */,
                                  int32_t n, uint64_t lo, uint64_t *__restrict__ keys,
                                  int32_t *__restrict__ rows_out /* may be null */)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows ? rows[p] : (int32_t)p;
    keys[p] = row_ok(i, n) ? (uint64_t)col[i] - lo : 0;
    if (rows_out) rows_out[p] = (int32_t)p;
}

// vs[p] = the value of sorted position p in the summing type A
template <typename T, typename A>
__global__ void gather_kernel(const T *__restrict__ data, const int32_t *__restrict__ rows, int32_t n, A *__restrict__ vs)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    vs[p] = row_ok(i, n) ? (A)data[i] : (A)0;
}

// ---- host ------------------------------------------------------------------------------------------------------
// One stable sort of a chain by col, whose values lie in lo .. hi, on the bits hi - lo needs.  `rows` is the order so
// far; the first sort of a chain starts from the identity, which it writes there.
template <typename T>
static int sort_by_column(const T *col, T lo, T hi, bool first, uint64_t *keys, uint64_t *keys_sorted, int32_t *rows,
                          int32_t *rows_out, int32_t n, hipStream_t s)
{
    PMI_LAUNCH(column_key_kernel<T>, n, s, col, first ? nullptr : rows, n, (uint64_t)lo, keys, first ? rows : nullptr);
    return sort_pairs(keys, keys_sorted, rows, rows_out, (size_t)n, bits_of((uint64_t)hi - (uint64_t)lo), s);
}

// a column of type T is summed in float when it is float32 and in double otherwise
template <typename T>
struct Column {
    using type = T;
    using sum_type = typename std::conditional<std::is_same<T, float>::value, float, double>::type;
};

// f(Column<T>()) for the T of a pmi_centers_type code
template <typename F>
static int with_column_type(int type, F &&f)
{
    switch (type) {
    case PMI_CENTERS_F32: return f(Column<float>());
    case PMI_CENTERS_F64: return f(Column<double>());
    case PMI_CENTERS_U32: return f(Column<uint32_t>());
    case PMI_CENTERS_I32: return f(Column<int32_t>());
    case PMI_CENTERS_U64: return f(Column<uint64_t>());
    default: return f(Column<int64_t>());
    }
}

}  // namespace rows
}  // namespace pmi
