// rbmc_plan.cpp -- host analysis of the RBMC variance estimators (rbmc_plan.h). No HIP.
//   (a) rbmc_build_sym: Symmetric(Q) row by row from the used triangle, O(nnz), once per handle;
//   (b) rbmc_build_plan: `_build_disjoint_subsets` (sequential by definition: a subset opens at the first node no earlier
//       subset has taken, and holds ALL stored neighbours of that node, taken or not) and `_build_enclosure_idcs`
//       (enclosure_size breadth-first rings, independent per subset: threads), src/solvers/rbmc.jl:93-117.
#include "rbmc_plan.h"

#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>

namespace gmrfx {

void rbmc_build_sym(const Symbolic &S, RbmcSym &R) {
    const i64 n = S.n;
    const bool lower = S.in_use != 0;
    std::vector<i64> cnt((size_t)n + 1, 0);
    for (i64 j = 0; j < n; j++)
        for (i64 p = S.in_colptr[j]; p < S.in_colptr[j + 1]; p++) {
            const i64 i = S.in_row[p];
            if (i == j) cnt[i + 1]++;
            else if (lower ? (i > j) : (i < j)) { cnt[i + 1]++; cnt[j + 1]++; }
        }
    for (i64 i = 0; i < n; i++) cnt[i + 1] += cnt[i];
    RbmcSym T;
    T.rowptr = cnt;
    T.col.assign((size_t)cnt[n], 0);
    T.pos.assign((size_t)cnt[n], 0);
    T.diag.assign((size_t)n, -1);
    std::vector<i64> fill(cnt.begin(), cnt.end() - 1);
    auto put = [&](i64 row, i64 c, i64 p) { const i64 q = fill[row]++; T.col[q] = (i32)c; T.pos[q] = p; };
    // two sweeps over the columns leave every row ascending when the caller's columns are: the part left of the diagonal, then the rest
    for (int sweep = 0; sweep < 2; sweep++)
        for (i64 j = 0; j < n; j++)
            for (i64 p = S.in_colptr[j]; p < S.in_colptr[j + 1]; p++) {
                const i64 i = S.in_row[p];
                if (lower) {
                    if (sweep == 0 && i >= j) { put(i, j, p); if (i == j) T.diag[i] = p; }     // row i, column j <= i
                    if (sweep == 1 && i > j) put(j, i, p);                                     // mirrored: row j, column i > j
                } else {
                    if (sweep == 0 && i < j) put(j, i, p);                                     // mirrored: row j, column i < j
                    if (sweep == 1 && i <= j) { put(i, j, p); if (i == j) T.diag[i] = p; }     // row i, column j >= i
                }
            }
    for (i64 i = 0; i < n; i++) {
        if (T.diag[i] < 0) throw std::invalid_argument("rbmc: row " + std::to_string(i) + " of Q has no stored diagonal entry");
        const i64 a = T.rowptr[i], b = T.rowptr[i + 1];
        if (!std::is_sorted(T.col.begin() + a, T.col.begin() + b)) {      // unsorted caller columns: order the row by column
            std::vector<std::pair<i32, i64>> e;
            for (i64 q = a; q < b; q++) e.push_back({T.col[q], T.pos[q]});
            std::stable_sort(e.begin(), e.end(), [](const std::pair<i32, i64> &x, const std::pair<i32, i64> &y) { return x.first < y.first; });
            for (i64 q = a; q < b; q++) { T.col[q] = e[q - a].first; T.pos[q] = e[q - a].second; }
        }
    }
    T.built = true;
    R = std::move(T);
}

namespace {
int plan_threads(i64 work) {
    const unsigned hc = std::thread::hardware_concurrency();
    const int cap = (int)std::min<unsigned>(8, std::max<unsigned>(1, hc / 2));
    return (int)std::max<i64>(1, std::min<i64>(cap, work >> 14));
}
template <class F> void for_blocks(i64 nb, i64 work, F &&fn) {
    const int T = plan_threads(work);
    if (T <= 1) { fn(0, nb, 0); return; }
    std::vector<std::thread> th;
    std::mutex mu;
    std::exception_ptr err;
    const i64 per = (nb + T - 1) / T;
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t]() {
            try {
                fn(std::min(nb, t * per), std::min(nb, (t + 1) * per), t);
            } catch (...) {
                std::lock_guard<std::mutex> g(mu);
                if (!err) err = std::current_exception();
            }
        });
    for (auto &x : th) x.join();
    if (err) std::rethrow_exception(err);
}
}  // namespace

void rbmc_build_plan(const RbmcSym &R, i64 n, int enclosure_size, RbmcPlan &P) {
    if (enclosure_size < 0) throw std::invalid_argument("rbmc: enclosure_size < 0 has no blocks");
    // the subset walk
    std::vector<i64> sptr{0};
    std::vector<i32> snodes;
    std::vector<i64> last((size_t)n, -1);
    {
        std::vector<uint8_t> visited((size_t)n, 0);
        for (i64 i = 0; i < n; i++) {
            if (visited[i]) continue;
            const i64 b = (i64)sptr.size() - 1;
            for (i64 q = R.rowptr[i]; q < R.rowptr[i + 1]; q++) {
                const i32 j = R.col[q];
                if (q > R.rowptr[i] && j == R.col[q - 1]) continue;      // (a duplicated entry is one neighbour)
                visited[j] = 1;
                last[j] = b;
                snodes.push_back(j);
            }
            const i64 sz = (i64)snodes.size() - sptr.back();
            if (sz > kRbmcMaxBlock)
                throw std::invalid_argument("rbmc: block " + std::to_string(b) + " has " + std::to_string(sz) + " rows (the subset of node " +
                                            std::to_string(i) + "); the device path factors blocks of at most 512 rows");
            sptr.push_back((i64)snodes.size());
        }
    }
    const i64 nb = (i64)sptr.size() - 1;
    // the enclosures: per subset, independent; one stamp array per thread marks the explored nodes
    std::vector<std::vector<i32>> enc((size_t)(enclosure_size > 0 ? nb : 0));
    if (enclosure_size > 0)
        for_blocks(nb, (i64)snodes.size() * enclosure_size, [&](i64 b0, i64 b1, int) {
            std::vector<i64> stamp((size_t)n, -1);
            std::vector<i32> frontier, next;
            for (i64 b = b0; b < b1; b++) {
                frontier.assign(snodes.begin() + sptr[b], snodes.begin() + sptr[b + 1]);
                for (i32 v : frontier) stamp[v] = b;
                i64 total = (i64)frontier.size();
                for (int ring = 0; ring < enclosure_size && !frontier.empty(); ring++) {
                    next.clear();
                    for (i32 v : frontier)
                        for (i64 q = R.rowptr[v]; q < R.rowptr[v + 1]; q++) {
                            const i32 j = R.col[q];
                            if (stamp[j] != b) { stamp[j] = b; next.push_back(j); }
                        }
                    std::sort(next.begin(), next.end());
                    total += (i64)next.size();
                    if (total > kRbmcMaxBlock)
                        throw std::invalid_argument("rbmc: block " + std::to_string(b) + " has " + (ring + 1 < enclosure_size ? "more than " : "") +
                                                    std::to_string(total) + " rows with enclosure_size = " + std::to_string(enclosure_size) +
                                                    "; the device path factors blocks of at most 512 rows (enclosure_size = 0 always stays available)");
                    enc[b].insert(enc[b].end(), next.begin(), next.end());
                    frontier.swap(next);
                }
            }
        });
    RbmcPlan T;
    T.enclosure = enclosure_size;
    T.block_ptr.assign((size_t)nb + 1, 0);
    T.n_interior.assign((size_t)nb, 0);
    for (i64 b = 0; b < nb; b++) {
        const i64 ns = sptr[b + 1] - sptr[b], sz = ns + (enclosure_size > 0 ? (i64)enc[b].size() : 0);
        T.n_interior[b] = (i32)ns;
        T.block_ptr[b + 1] = T.block_ptr[b] + sz;
        T.max_block = std::max(T.max_block, sz);
        T.order[rbmc_class((int)sz)].push_back((i32)b);
    }
    const i64 tot = T.block_ptr[nb];
    T.rows.assign((size_t)tot, 0);
    T.owner.assign((size_t)tot, 0);
    T.eptr.assign((size_t)tot + 1, 0);
    for (i64 b = 0; b < nb; b++) {
        i64 o = T.block_ptr[b];
        for (i64 q = sptr[b]; q < sptr[b + 1]; q++, o++) { T.rows[o] = snodes[q]; T.owner[o] = last[snodes[q]] == b ? 1 : 0; }
        if (enclosure_size > 0) for (i32 v : enc[b]) T.rows[o++] = v;
    }
    for (i64 r = 0; r < tot; r++) T.eptr[r + 1] = T.eptr[r] + (R.rowptr[T.rows[r] + 1] - R.rowptr[T.rows[r]]);
    T.loc.assign((size_t)T.eptr[tot], -1);
    for_blocks(nb, T.eptr[tot], [&](i64 b0, i64 b1, int) {
        std::vector<i32> where((size_t)n, -1);
        for (i64 b = b0; b < b1; b++) {
            const i64 r0 = T.block_ptr[b], sz = T.block_ptr[b + 1] - r0;
            for (i64 k = 0; k < sz; k++) where[T.rows[r0 + k]] = (i32)(sz - 1 - k);      // S last
            for (i64 k = 0; k < sz; k++) {
                const i64 g = T.rows[r0 + k], e0 = T.eptr[r0 + k];
                for (i64 q = R.rowptr[g]; q < R.rowptr[g + 1]; q++) T.loc[e0 + (q - R.rowptr[g])] = where[R.col[q]];
            }
            for (i64 k = 0; k < sz; k++) where[T.rows[r0 + k]] = -1;
        }
    });
    T.serial = P.serial + 1;      // the device's copy of an earlier plan is stale
    P = std::move(T);
}

}  // namespace gmrfx
