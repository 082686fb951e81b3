// Shared encodings (DESIGN.md "shared encodings"): the rows of a batch that read the same crop are given that crop's
// encoder output by copying it.  A pure bandwidth kernel: out[r] = in[src_of_row[r]] for r < rows, every row `chunks`
// 16-byte pieces (197 x 768 elements: 18,912 in bf16, 37,824 in fp32), one piece per lane, loads and stores coalesced.
// `in` and `out` are different buffers: a gather in place is wrong (row 0 may read source 2 while row 2 is being written).
#pragma once
#include "common.h"

constexpr int EXPAND_THREADS = 256;

// grid = rows * blocks_per_row, blocks_per_row = ceil(chunks / EXPAND_THREADS): block b copies pieces of row b / blocks_per_row.
// The row's source index is one wave-uniform load per block.  Rows >= rows are never written (the grid has no such block), a
// source outside [0, n_src) copies nothing (the host validates the indices; this is the second fence).
__global__ __launch_bounds__(EXPAND_THREADS) void enc_expand_kernel(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                                    const int* __restrict__ src_of_row, int n_src, int rows,
                                                                    int chunks, int blocks_per_row) {
    const int row = blockIdx.x / blocks_per_row;
    const int piece = (blockIdx.x - row * blocks_per_row) * EXPAND_THREADS + threadIdx.x;
    if (row >= rows || piece >= chunks) return;
    const int src = src_of_row[row];
    if ((unsigned)src >= (unsigned)n_src) return;
    out[(size_t)row * chunks + piece] = in[(size_t)src * chunks + piece];
}
