// The LDS layout of the wide resident CROWN kernel (crown_wide.hpp, hidden layers up to 128 wide), stated once: how a backward pass
// is cut into slabs of rows, where element (row, column) of a slab's two coefficient matrices and entry t of every vector sits, and
// how many bytes the kernel is launched with.  Plain C++ (a test compiles it for the host alone and enumerates it); crown_wide.hpp
// includes it for both sides.
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#define NNSDP_CW_HD __host__ __device__
#else
#define NNSDP_CW_HD
#endif

namespace nnsdp {

static constexpr int kCwRows = 64;      // rows of a slab: the row stride of cb_idx, and the widest xdims[0], xdims[K] and nlit
static constexpr int kCwCols = 128;     // columns of a slab: the widest hidden layer

// a pass of nout rows runs in cw_slabs(nout) slabs; slab s holds the rows 64 s .. 64 s + cw_slab_rows(nout, s) - 1
NNSDP_CW_HD inline int cw_slabs(const int nout) { return (nout + kCwRows - 1) / kCwRows; }
NNSDP_CW_HD inline int cw_slab_rows(const int nout, const int s) { return nout - kCwRows * s < kCwRows ? nout - kCwRows * s : kCwRows; }

// element (column t, row i of the slab) inside one matrix: cb_idx of crown_batch.hpp, [column][row] with the 16-row tiles of odd
// columns swapped, row stride 64
NNSDP_CW_HD inline int cw_idx(const int t, const int i) { return t * kCwRows + (i ^ ((t & 1) << 4)); }

// offsets in doubles from the start of the dynamic LDS: the two matrices, then the vectors
static constexpr int kCwMat = kCwRows * kCwCols;        // one matrix
static constexpr int kCwOffDu = 2 * kCwMat;             // 128: upper slope
static constexpr int kCwOffDl = kCwOffDu + kCwCols;     // 128: lower slope
static constexpr int kCwOffBu = kCwOffDl + kCwCols;     // 128: upper relaxation's bias
static constexpr int kCwOffBj = kCwOffBu + kCwCols;     // 128: the layer's bias b_j
static constexpr int kCwOffC = kCwOffBj + kCwCols;      // 64: box centre
static constexpr int kCwOffR = kCwOffC + kCwRows;       // 64: box radius
static constexpr int kCwOffRes = kCwOffR + kCwRows;     // 2 x 64: a slab's lower / upper results
static constexpr int kCwOffBl = kCwOffRes + 2 * kCwRows;   // 128, Tanh only: the lower relaxation's bias
static constexpr int kCwDoubles = kCwOffBl;             // ReLU
static constexpr int kCwDoublesTanh = kCwOffBl + kCwCols;
static constexpr size_t kCwLdsBytes = (size_t)kCwDoubles * sizeof(double);          // 137 216 B
static constexpr size_t kCwLdsBytesTanh = (size_t)kCwDoublesTanh * sizeof(double);  // 138 240 B

NNSDP_CW_HD inline int cw_mat_off(const int mat, const int t, const int i) { return mat * kCwMat + cw_idx(t, i); }

}  // namespace nnsdp
