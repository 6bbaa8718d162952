// selinv_offsets.h -- where an entry of the selected inverse lives in the panel storage (Device::d_Z_), from the symbolic structure
// alone (host code, no HIP). Shared by the selected-inverse entry points (api_selinv.cpp) and the gradient tables (device_grad.cpp).
#pragma once
#include <algorithm>
#include <exception>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <vector>

#include "symbolic.h"

namespace gmrfx {

// Host-side planning loops (offset lookups into the supernodal structure) over [0, n): split over a few threads
// when long; fn(lo, hi) must only write its own range. Exceptions inside fn are collected and rethrown.
template <class F> inline void parallel_ranges(i64 n, F &&fn) {
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    if (n < 200000 || hw == 1) { fn((i64)0, n); return; }
    std::vector<std::thread> th;
    th.reserve(hw);      // no reallocation (and so no bad_alloc with joinable threads alive) inside the loop
    std::vector<std::exception_ptr> err(hw);
    for (unsigned t = 0; t < hw; t++) {
        auto job = [&, t] { try { fn(n * t / hw, n * (t + 1) / hw); } catch (...) { err[t] = std::current_exception(); } };
        try { th.emplace_back(job); } catch (const std::system_error &) { job(); }     // no thread to be had: inline
    }
    for (auto &x : th) x.join();
    for (auto &e : err) if (e) std::rethrow_exception(e);
}

// offset of Sigma(i, j) (original indices) in the selected-inverse panels, -1 outside the factor pattern
inline long long z_offset(const Symbolic &S, i64 i, i64 j) {
    i32 a = S.iperm[i], b = S.iperm[j];
    if (a < b) std::swap(a, b);
    const i32 s = S.col2super[b];
    const i32 *rows = S.rows.data() + S.rowptr[s];
    const i32 r = S.nrows(s);
    const i32 *it = std::lower_bound(rows, rows + r, a);
    if (it == rows + r || *it != a) return -1;
    if (S.shard_plan && S.owner[s] != S.shard_rank) return (long long)S.panelptr[S.nsuper];      // another rank's panel: the zeroed slack word
    return (long long)(S.panelptr[s] + (i64)(b - S.sfirst[s]) * S.ld[s] + (it - rows));
}

// z_offset of every entry of a CSC pattern (colptr monotone with colptr[0] == base: check_compressed_ptr for a caller's), in the
// pattern's order; Row: the pattern's row index type
template <class Row>
inline std::vector<long long> z_offsets_csc(const Symbolic &S, int64_t ncol, const int64_t *colptr, const Row *rowval, int32_t base) {
    std::vector<long long> off((size_t)(colptr[ncol] - base));
    parallel_ranges(ncol, [&](i64 lo, i64 hi) {
        for (i64 j = lo; j < hi; j++)
            for (i64 p = colptr[j] - base; p < colptr[j + 1] - base; p++) {
                i64 i = (i64)rowval[p] - base;
                if (i < 0 || i >= S.n) throw std::invalid_argument("rowval out of range");
                off[p] = z_offset(S, i, j);
            }
    });
    return off;
}

}  // namespace gmrfx
