// rbmc_plan.h -- host analysis of the Rao-Blackwellised Monte Carlo variance estimators (rbmc_plan.cpp, no HIP): the row-wise
// image of symmetric Q and the blocks of BlockRBMCStrategy (reference: src/solvers/rbmc.jl:90-158). Built lazily and kept on
// the handle; Device::rbmc_var uploads the tables as they are.
#pragma once
#include <cstdint>
#include <vector>

#include "symbolic.h"

namespace gmrfx {

constexpr int kRbmcMaxBlock = 512;     // rows of the largest block the device path factors (the limit of kl_cholesky)
constexpr int kRbmcClasses = 4;        // size classes of the block kernel: <= 32, <= 64, <= 128 rows (LDS), <= 512 (global scratch)
inline int rbmc_class(int rows) { return rows <= 32 ? 0 : (rows <= 64 ? 1 : (rows <= 128 ? 2 : 3)); }

// Symmetric(Q) row by row, from the stored triangle that defines Q (Symbolic::in_use), mirrored; columns ascending within a row.
// Entries of the other triangle are ignored even where they are stored. Explicit zeros are entries (what `findnz` returns).
struct RbmcSym {
    bool built = false;
    std::vector<i64> rowptr;     // n+1
    std::vector<i32> col;        // 32-bit columns
    std::vector<i64> pos;        // position of the entry in the caller's nzval
    std::vector<i64> diag;       // n: position of Q_ii in the caller's nzval
};

// The blocks of one enclosure size. Block b = rows[block_ptr[b] .. block_ptr[b+1]): its subset S first (n_interior[b] rows, ascending),
// then the enclosure ring by ring (ascending inside a ring). owner = 1 where b is the LAST block whose subset holds the node:
// the reference's `var_estimate[interior] .=` lets the last subset decide, so exactly one block writes every node.
// The kernels factor a block with S LAST: local row l of a block is rows[block_ptr[b] + nb - 1 - l]; loc holds, for every entry of
// every block row (in the order of RbmcSym's row), the local row of its column inside the block, or -1 for a column outside.
struct RbmcPlan {
    int enclosure = -2;          // -2: nothing built
    unsigned long long serial = 0;
    std::vector<i64> block_ptr;
    std::vector<i32> rows, n_interior;
    std::vector<uint8_t> owner;
    std::vector<i64> eptr;       // total rows + 1: first entry of a block row in loc
    std::vector<i32> loc;
    std::vector<i32> order[kRbmcClasses];    // blocks by size class
    i64 max_block = 0;
    i64 nblocks() const { return block_ptr.empty() ? 0 : (i64)block_ptr.size() - 1; }
};

// Throws std::invalid_argument (message names the row) when a row has no stored diagonal entry.
void rbmc_build_sym(const Symbolic &S, RbmcSym &R);
// Throws std::invalid_argument naming the block and its size when a block has more than kRbmcMaxBlock rows; P is then unchanged.
void rbmc_build_plan(const RbmcSym &R, i64 n, int enclosure_size, RbmcPlan &P);

}  // namespace gmrfx
