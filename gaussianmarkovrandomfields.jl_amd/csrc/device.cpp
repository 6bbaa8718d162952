// device.cpp -- HBM residency of the symbolic structure and the level-scheduled numeric
// drivers (factorise, sweeps, log-determinant, selected inverse). Compiled with hipcc.
#include "device.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <stdexcept>
#include <thread>
#include <type_traits>

#include "kernels.h"

namespace gmrfx {

void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}
#define HC(x) hip_check((x), #x)

static constexpr size_t kPairSlackBytes = 16;
static constexpr size_t kChunkSlack = 16 * 320;      // doubles behind the factor storage (sweep_chunk.hip reads tiles without clamps)
template <class T> T *Device::dalloc(size_t count) {
    // 16 bytes of slack behind every array: kernels that load rows in pairs (16 bytes per lane) may read one element
    // past the last one; the value is never used, but the address must be mapped
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T) + kPairSlackBytes;
    HC(hipMalloc(&p, bytes));
    allocs_.push_back(p);
    bytes_total += (double)bytes;
    return (T *)p;
}

// Grows a buffer that may be replaced during the life of the handle: the NEW buffer is allocated first, so that a failed
// allocation (exception) leaves the old one and its capacity valid; callers raise their *_cap_ only after the return. The old
// one is released once nothing in flight can still read it.
template <class T> static void regrow(DevBuf<T> &buf, size_t count, double *ledger) {
    DevBuf<T> fresh;
    fresh.alloc(count, ledger);
    if (buf) HC(hipDeviceSynchronize());
    buf = std::move(fresh);
}

// (the members release what they own, buffers and events before the streams: see the declarations)
Device::~Device() {
    if (stream) { (void)hipStreamSynchronize(stream); }
    for (void *p : allocs_) (void)hipFree(p);
}

// The caller's stream becomes the main stream (sharded drivers: torch's current stream, so that the library's kernels,
// torch's copies and the RCCL operations torch enqueues are ordered by the stream itself and no host-side synchronisation
// is needed between a phase and the exchange behind it); async: the phase entry points return after enqueueing.
void Device::set_external_stream(hipStream_t s, bool use, bool async) {
    HC(hipSetDevice(device));
    HC(hipStreamSynchronize(stream));
    stream = use ? s : own_stream_;
    async_phases_ = use && async;
}

void Device::init(const Symbolic &S, int dev) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) throw std::runtime_error("no HIP device available (libgmrfx has no CPU fallback)");
    if (dev < 0) HC(hipGetDevice(&dev));
    if (dev >= count) throw std::runtime_error("HIP device ordinal out of range");
    device = dev;
    HC(hipSetDevice(device));
    {
        // the main stream carries the dependent chain of the factorisation / sweeps: highest priority; the side
        // stream (dense inverses) only fills idle capacity: lowest
        int lo = 0, hi = 0;
        HC(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // (Measured and settled in round 4, DESIGN.md section 3: no priorities, idle streams between the handle's streams, a CU mask on
        //  the side stream -- none of them helps; the three streams are created back to back: three distinct hardware queues.)
        own_stream_.create(hipStreamNonBlocking, hi);
        stream = own_stream_;
        stream2.create(hipStreamNonBlocking, lo);
        stream3.create(hipStreamNonBlocking, hi);
    }
    env_ = read_env_knobs();
    inv_cap_ = env_.inv_cap;
    ev_fact_.create(hipEventDisableTiming);
    ev_inv_.create(hipEventDisableTiming);
    for (auto &ev : ev_) ev.create();
    for (auto &l : ev_lane_) for (auto &ev : l) ev.create();
    {
        int khz = 0;
        HC(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device));
        if (khz <= 0) throw std::runtime_error("the device reports no wall clock rate");
        wall_clock_khz_ = khz;
    }
    // the pivot word (+ one of padding), then a pair of 64-bit clock stamps per SYRK slot: one slot per level at most
    h_info_.alloc(kInfoWords + 4 * (long long)S.nlevels);
    std::fill_n((int *)h_info_, kInfoWords + 4 * (long long)S.nlevels, 0);
    h_info_[0] = INT_MAX;
    ev_ready_.create(hipEventDisableTiming);
    ev_ready2_.create(hipEventDisableTiming);
    ev_done1_.create(hipEventDisableTiming);
    upload(S);
}

void Device::upload(const Symbolic &S) {
    S_ = &S;
    const DevicePlan P = build_device_plan(S, PlanOptions{env_.syrk_xcd});
    // a device copy of a host vector (the analysis' int64_t offsets become the kernels' long long: the same bytes). The copies
    // read the host vectors until the synchronisation at the end, while P and S still hold them.
    auto up = [&](const auto &host) {
        using T = typename std::decay_t<decltype(host)>::value_type;
        using D = std::conditional_t<std::is_same<T, i64>::value, long long, T>;
        static_assert(sizeof(D) == sizeof(T), "a device array holds the same bytes as its host vector");
        D *p = dalloc<D>(host.size());
        if (!host.empty()) HC(hipMemcpyAsync(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        return p;
    };
    levels_ = P.levels; swlevels_ = P.swlevels; sel_max_cols_ = P.sel_max_cols; sel_max_trail_ = P.sel_max_trail;
    inv_maxc_ = P.inv_maxc; inv_nact_ = P.inv_nact; inv_lvl_first_ = P.inv_lvl_first; inv_lvl_maxc_ = P.inv_lvl_maxc; inv_lvl_nact_ = P.inv_lvl_nact;
    fc_levelptr_ = P.fc_levelptr; fc_maxtrail_ = P.fc_maxtrail;
    std::copy_n(P.wave_first, kWaveClasses, wave_first_); std::copy_n(P.wave_count, kWaveClasses, wave_count_); std::copy_n(P.nsub_cls, 3, nsub_cls_);
    bottom_top_level_ = P.bottom_top_level; fused_gate_level_ = P.fused_gate_level; first_multiblock_level_ = P.first_multiblock_level;
    syrk_flops = P.syrk_flops; sum_trail_ = P.sum_trail; l_size_ = P.l_size; nq_ = P.nq; nswt_ = P.nswt; nswc_ = P.nswc;

    ds_.n = (int)S.n;
    ds_.nsuper = S.nsuper;
    ds_.sfirst = up(S.sfirst); ds_.rowptr = up(S.rowptr); ds_.rows = up(S.rows); ds_.rel = up(S.rel);
    ds_.panelptr = up(S.panelptr); ds_.ld = up(S.ld); ds_.cbptr = up(S.cbptr);
    d_zbptr_ = up(S.zbptr);
    d_selrec_ = up(P.selrec);
    ds_.childptr = up(S.childptr); ds_.children = up(S.children); ds_.sparent = up(S.sparent);
    ds_.qptr = up(S.qptr); ds_.qsrc = up(P.qsrc); ds_.qdst = up(P.qdst); ds_.qcol = up(P.qcol); ds_.qcolptr = up(P.qcolptr);
    d_nzp_ = dalloc<double>((size_t)std::max<long long>(nq_, 1));
    ev_nzp_.create(hipEventDisableTiming);
    ev_nzp0_.create(hipEventDisableTiming);
    ds_.wptr = up(S.wptr);
    ds_.edge = up(P.edge); ds_.etile = up(P.etile); ds_.erow = up(P.erow);
    ds_.diagoff = up(S.diagoff); ds_.perm = up(S.perm);
    d_iperm_ = up(S.iperm);
    if (S.shard_plan) {
        d_owncol_ = up(P.owncol);
        ds_.foreign_parent = up(P.foreign_parent);
        d_fchild_ = up(P.fchild);
    }
    ds_.lrow = up(S.lrow);
    d_sw_levellist_ = up(S.sw_levellist);
    if (nswc_ > 0) {
        d_swc_fwd_ = up(S.swc_fwd); d_swc_bwd_ = up(S.swc_bwd);
        d_swc_listf_ = up(P.swc_listf); d_swc_listb_ = up(P.swc_listb);
        d_dtile_ = dalloc<double>((size_t)nswc_ * 256);
    }
    d_swt_ = up(P.swt);
    d_wave_order_ = up(P.wave_order);
    d_levellist_ = up(S.levellist); d_levellist2_ = up(P.levellist2);
    d_sub_first_ = up(S.sub_first); d_sub_last_ = up(S.sub_last);
    d_sel_levellist_ = up(S.sel_levellist);
    d_frec_ = up(P.frec); d_sel_frec_ = up(P.sel_frec); d_frec2_ = up(P.frec2);
    d_invlist_ = up(P.invlist);
    for (const auto &off : P.inv_toff) d_inv_toff_.push_back(up(off));
    d_invT_ = dalloc<double>((size_t)std::max<long long>(P.inv_tsize, 1));
    if (!P.inv_lvl_list.empty()) d_inv_lvl_list_ = up(P.inv_lvl_list);
    for (const auto &off : P.inv_lvl_toff) d_inv_lvl_toff_.push_back(up(off));
    d_syrk_recs_ = up(P.syrk_recs); d_fwd_recs_ = up(P.fwd_recs); d_arec_ = up(P.arec);
    {
        // where the tiles of k_syrk_cb_rec leave their times (two words each), and per level its tiles and its SYRK slot: the slots
        // go to the levels with big fronts that have trailing rows, in level order (factor_levels counts them the same way)
        std::vector<SyrkLevelTimes> lt(levels_.size());
        int slot = 0;
        for (size_t l = 0; l < levels_.size(); l++) {
            const LevelInfo &L = levels_[l];
            const long long end = l + 1 < levels_.size() ? levels_[l + 1].syrk_off : (long long)P.syrk_recs.size();
            const bool timed = L.nbig() > 0 && L.max_trail > 0;
            lt[l] = SyrkLevelTimes{L.syrk_off, env_.syrk_xcd && timed ? (int)(end - L.syrk_off) : 0, timed ? slot++ : -1};
        }
        d_syrk_level_times_ = up(lt);
        d_syrk_times_ = dalloc<unsigned long long>(2 * P.syrk_recs.size());
    }

    // INVARIANT (pair loads): the kernels that read operand rows in 16-byte pairs (sweep_front.hip, k_syrk_cb_rec, selinv.hip)
    // may read ONE double past a column's last row; for the last column of the last panel that is element l_size_ of the
    // buffer. Every buffer that holds panels (d_L_, d_Z_, a clone) is therefore allocated through dalloc (16 bytes of
    // slack) and zeroed INCLUDING the slack, so the extra element is mapped and finite (it only ever meets a 0.0 mask).
    static_assert(kPairSlackBytes >= sizeof(double), "pair loads read one element past the end");
    // (the chunk kernels of the sweep tasks read whole 16-column / 16-row tiles from a chunk's first element without clamps: for
    //  the last task panel of the buffer that is up to 16 columns of <= 304 rows past its end -- mapped, zero, never used)
    d_L_ = dalloc<double>((size_t)l_size_ + kChunkSlack);
    d_cb_ = dalloc<double>((size_t)S.cb_arena);
    d_nz_ = dalloc<double>((size_t)S.nnz_in);
    d_info_ = dalloc<int>((size_t)kInfoWords + 4 * (size_t)S.nlevels);      // (the same layout as h_info_)
    d_part_ = dalloc<double>(1024 + 8);
    HC(hipMemsetAsync(d_L_, 0, ((size_t)l_size_ + kChunkSlack) * sizeof(double) + kPairSlackBytes, stream));
    HC(hipStreamSynchronize(stream));
}

void Device::clone_from(const Device &o, const Symbolic &S) {
    init(S, o.device);
    inv_cap_ = o.inv_cap_;
    inv_cap_decided_ = o.inv_cap_decided_;
    ms_inv_decide = o.ms_inv_decide;
    if (o.factorized) {
        HC(hipMemcpyAsync(d_L_, o.d_L_, (size_t)l_size_ * sizeof(double), hipMemcpyDeviceToDevice, stream));
        HC(hipMemcpyAsync(d_info_, o.d_info_, sizeof(int), hipMemcpyDeviceToDevice, stream));
        HC(hipStreamSynchronize(stream));
        factorized = true;
        inverse_pending = true;   // the copy may predate the source's lazy inverse: recompute on demand
    }
}

// ---- host I/O of the pipelined factor + solve call (gmrfx_refactorize_solve with HOST B / X: what the reference's
// workspace_solve(ws, B::Matrix) hands over, src/workspace/backend.jl:207-209) ---------------------------------------------
// n x nrhs doubles each way (2 x 512 MB at cfg 2: ~9 ms each at the link's 57 GB/s, tools/pcie_probe.py) around a 14 ms step.
// MEASURED (tools/host_io_step.py, cfg 2): the upload must NOT run beside the factorisation. Next to a 512 MB transfer on
// another queue the factorisation takes 18-24 ms instead of 11.7 when the DMA engines move the bytes, and 25-30 ms when ONE
// long kernel of 16 / 48 / 128 workgroups reads the page-locked buffer over PCIe (k_stream_copy; one launch, no DMA packets) --
// the panel chain's ~500 dependent dispatches lose the command processor to whatever else is active (tools/interference.py
// shows the same for every kind of concurrent work). So the transfers are serial -- B in, then the pipelined step, then X out --
// at the full rate of the DMA engines, and what is overlapped is the host side: pageable memory is staged through a page-locked
// buffer of the handle by several host threads (a single thread moves ~10 GB/s, the link 57), slice k's staging beside the DMA
// of slice k-1, and on the way out slice k's copy to the caller's array beside the DMA of slice k+1. Page-locked caller memory
// (page-locked through HIP, torch pin_memory) is handed to the DMA engine as it is.
// true for anything the DMA engines take as it is: page-locked host memory -- and device / managed memory handed to a host entry
// point by mistake or convenience (the copy is then device-to-device; a host thread must never memcpy from it)
static bool host_ptr_is_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}
static int host_io_threads() {
    static const int nt = [] {
        const unsigned hc = std::thread::hardware_concurrency();
        return (int)std::min<unsigned>(8, std::max<unsigned>(1, hc / 2));
    }();
    return nt;
}
// Pageable host memory is staged through a RING of page-locked slices that belongs to the handle: kIoRing slices of
// kIoSliceBytes (128 MB per handle, whatever the size of the right-hand sides -- a WorkspacePool keeps one handle per thread; round 4
// held n x nrhs doubles, 512 MB at cfg 2). Slice k uses slot k mod kIoRing once slice k - kIoRing has left it.
static constexpr long long kIoSliceBytes = 16ll << 20;     // staging granularity
static constexpr int kIoRing = 8;

// count doubles copied by up to T host threads (used for values that must arrive before anything can start)
static void parallel_memcpy(double *dst, const double *src, long long count) {
    const int T = (int)std::min<long long>(host_io_threads(), std::max<long long>(1, count >> 18));
    if (T <= 1) { std::memcpy(dst, src, (size_t)count * sizeof(double)); return; }
    std::vector<std::thread> th;
    const long long per = (count + T - 1) / T;
    for (int t = 1; t < T; t++) {
        const long long a = t * per, e = std::min(count, a + per);
        if (a < e) th.emplace_back([=] { std::memcpy(dst + a, src + a, (size_t)(e - a) * sizeof(double)); });
    }
    std::memcpy(dst, src, (size_t)std::min(per, count) * sizeof(double));
    for (auto &x : th) x.join();
}

// How a column-major n x nrhs host array is cut into slices of at most `slice_bytes` for the staging ring: whole columns while a
// column fits a slice (cols_per of them), otherwise ppc row pieces per column of rows_per rows each -- a slot never holds more than
// slice_bytes / 8 doubles whatever n is (round 5 clamped the RING but not the slot: from n > 2^21 on, slots 6 / 7 lay behind the
// page-locked buffer). Pure arithmetic, exported as gmrfx_host_io_plan and walked on the CPU (tests/test_cabi.py, tools/sanitize_host.cpp).
HostIoPlan host_io_plan(long long n, long long nrhs, long long slice_bytes) {
    HostIoPlan p;
    const long long slice_doubles = std::max<long long>(1, slice_bytes / (long long)sizeof(double));
    n = std::max<long long>(n, 1);
    if (n <= slice_doubles) {
        p.cols_per = slice_doubles / n; p.ppc = 1; p.rows_per = n;
        p.slot_doubles = p.cols_per * n;
        p.nsl = (nrhs + p.cols_per - 1) / p.cols_per;
    } else {
        p.cols_per = 1; p.ppc = (n + slice_doubles - 1) / slice_doubles; p.rows_per = (n + p.ppc - 1) / p.ppc;
        p.slot_doubles = p.rows_per;
        p.nsl = nrhs * p.ppc;
    }
    p.reserve = std::min<long long>(p.nsl, kIoRing) * p.slot_doubles;
    return p;
}
HostIoPlan host_io_plan_dir(long long n, long long nrhs, int download) { return host_io_plan(n, nrhs, download ? kIoSliceBytes / 2 : kIoSliceBytes); }
// slice k of the plan: columns [j0, j0 + nc) x rows [r0, r0 + nr)
static inline void host_io_slice(const HostIoPlan &p, long long k, long long n, long long nrhs, long long &j0, long long &nc, long long &r0, long long &nr) {
    if (p.ppc == 1) { j0 = k * p.cols_per; nc = std::min(p.cols_per, nrhs - j0); r0 = 0; nr = n; }
    else { j0 = k / p.ppc; nc = 1; r0 = (k % p.ppc) * p.rows_per; nr = std::max<long long>(0, std::min(p.rows_per, n - r0)); }
}

void Device::host_io_reserve(long long count) {
    if (!stream_io_) {
        stream_io_.create(hipStreamNonBlocking);
        ev_up_.create(hipEventDisableTiming);
        ev_x_.create(hipEventDisableTiming);
    }
    if (count <= h_stage_.cap()) return;
    if (h_stage_) HC(hipStreamSynchronize(stream_io_));       // (only the copy stream ever touches it)
    h_stage_.alloc(count);
}

// Q's values from a host array to d_nz_, ahead of the factorisation (nothing else runs yet: plain DMA)
void Device::host_upload_values(const double *nzval) {
    const long long cnt = S_->nnz_in;
    if (host_ptr_is_pinned(nzval)) {
        HC(hipMemcpyAsync(d_nz_, nzval, (size_t)cnt * sizeof(double), hipMemcpyDefault, stream));
        return;
    }
    if (!h_nzstage_) h_nzstage_.alloc(cnt);
    HC(hipStreamSynchronize(stream));                 // (an earlier call's copy out of the staging buffer has finished long ago; cheap)
    parallel_memcpy(h_nzstage_, nzval, cnt);
    HC(hipMemcpyAsync(d_nz_, h_nzstage_, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, stream));
}

// B (host, column-major n x nrhs, leading dimension ldb) -> d_dst (device, column-major, leading dimension n), on the copy
// stream; returns after every copy has been ENQUEUED and ev_up_ recorded behind the last one.
void Device::host_upload(const double *B, long long ldb, long long nrhs, double *d_dst) {
    const long long n = S_->n;
    host_io_reserve(0);
    if (host_ptr_is_pinned(B)) {
        if (ldb == n) HC(hipMemcpyAsync(d_dst, B, (size_t)(n * nrhs) * sizeof(double), hipMemcpyDefault, stream_io_));
        else HC(hipMemcpy2DAsync(d_dst, n * sizeof(double), B, ldb * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDefault, stream_io_));
        HC(hipEventRecord(ev_up_, stream_io_));
        return;
    }
    // column slices; slice k is staged by host thread k mod T into ring slot k mod kIoRing (once the DMA of slice k - kIoRing has
    // left that slot), then handed to the DMA engine
    const HostIoPlan pl = host_io_plan(n, nrhs, kIoSliceBytes);
    const long long slot_doubles = pl.slot_doubles, nsl = pl.nsl;
    host_io_reserve(pl.reserve);
    const int T = (int)std::min<long long>(host_io_threads(), nsl);
    while ((int)ev_ring_.size() < kIoRing) { Event e; e.create(hipEventDisableTiming); ev_ring_.push_back(std::move(e)); }
    std::vector<std::atomic<int>> posted((size_t)nsl);
    for (auto &a : posted) a.store(0);
    std::vector<std::thread> th;
    std::exception_ptr err;
    std::atomic<bool> failed{false};
    const int dev = device;
    auto work = [&](int t) {
        try {
            HC(hipSetDevice(dev));
            for (long long k = t; k < nsl && !failed.load(); k += T) {
                long long j0, nc, r0, nr;
                host_io_slice(pl, k, n, nrhs, j0, nc, r0, nr);
                const int slot = (int)(k % kIoRing);
                if ((slot + 1) * slot_doubles > h_stage_.cap() || nc * nr > slot_doubles) throw std::runtime_error("host_upload: slice leaves the staging ring");
                if (k >= kIoRing) {         // the slot's previous slice: its copy has been enqueued (posted), now wait until it has run
                    while (!posted[(size_t)(k - kIoRing)].load(std::memory_order_acquire)) { if (failed.load()) return; std::this_thread::yield(); }
                    HC(hipEventSynchronize(ev_ring_[slot]));
                }
                double *st = h_stage_ + slot * slot_doubles;
                for (long long j = 0; j < nc; j++)
                    std::memcpy(st + j * nr, B + (j0 + j) * ldb + r0, (size_t)nr * sizeof(double));
                if (nc * nr > 0) HC(hipMemcpyAsync(d_dst + j0 * n + r0, st, (size_t)(nc * nr) * sizeof(double), hipMemcpyHostToDevice, stream_io_));
                HC(hipEventRecord(ev_ring_[slot], stream_io_));
                posted[(size_t)k].store(1, std::memory_order_release);
            }
        } catch (...) {
            if (!failed.exchange(true)) err = std::current_exception();
        }
    };
    for (int t = 1; t < T; t++) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    if (err) std::rethrow_exception(err);
    HC(hipEventRecord(ev_up_, stream_io_));
}

// d_src (device, column-major n x nrhs, leading dimension n; final once `after` has passed) -> X (host); returns when X is complete
void Device::host_download(const double *d_src, long long nrhs, double *X, long long ldx, hipStream_t after) {
    const long long n = S_->n;
    host_io_reserve(0);
    // the copies are enqueued only once their source is final: a device-to-host copy that has to wait for an event on another
    // stream took 21 ms instead of 9 here (512 MB; the runtime leaves the DMA path for it)
    HC(hipStreamSynchronize(after));
    if (host_ptr_is_pinned(X)) {
        if (ldx == n) HC(hipMemcpyAsync(X, d_src, (size_t)(n * nrhs) * sizeof(double), hipMemcpyDefault, stream_io_));
        else HC(hipMemcpy2DAsync(X, ldx * sizeof(double), d_src, n * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDefault, stream_io_));
        HC(hipStreamSynchronize(stream_io_));
        return;
    }
    // slice k: device -> ring slot k mod kIoRing (once slice k - kIoRing has been copied out of it) -> the caller's array; host
    // thread k mod T does all three steps, up to T transfers in flight
    const HostIoPlan pl = host_io_plan(n, nrhs, kIoSliceBytes / 2);
    const long long slot_doubles = pl.slot_doubles, nsl = pl.nsl;
    host_io_reserve(pl.reserve);
    while ((int)ev_ring_.size() < kIoRing) { Event e; e.create(hipEventDisableTiming); ev_ring_.push_back(std::move(e)); }
    std::vector<std::atomic<int>> done((size_t)nsl);
    for (auto &a : done) a.store(0);
    const int T = (int)std::min<long long>(std::min<long long>(host_io_threads(), kIoRing), nsl);
    std::vector<std::thread> th;
    std::exception_ptr err;
    std::atomic<bool> failed{false};
    const int dev = device;
    auto work = [&](int t) {
        try {
            HC(hipSetDevice(dev));
            for (long long k = t; k < nsl && !failed.load(); k += T) {
                long long j0, nc, r0, nr;
                host_io_slice(pl, k, n, nrhs, j0, nc, r0, nr);
                const int slot = (int)(k % kIoRing);
                if ((slot + 1) * slot_doubles > h_stage_.cap() || nc * nr > slot_doubles) throw std::runtime_error("host_download: slice leaves the staging ring");
                if (k >= kIoRing)
                    while (!done[(size_t)(k - kIoRing)].load(std::memory_order_acquire)) { if (failed.load()) return; std::this_thread::yield(); }
                double *st = h_stage_ + slot * slot_doubles;
                if (nc * nr > 0) HC(hipMemcpyAsync(st, d_src + j0 * n + r0, (size_t)(nc * nr) * sizeof(double), hipMemcpyDeviceToHost, stream_io_));
                HC(hipEventRecord(ev_ring_[slot], stream_io_));
                HC(hipEventSynchronize(ev_ring_[slot]));
                for (long long j = 0; j < nc; j++)
                    std::memcpy(X + (j0 + j) * ldx + r0, st + j * nr, (size_t)nr * sizeof(double));
                done[(size_t)k].store(1, std::memory_order_release);
            }
        } catch (...) {
            if (!failed.exchange(true)) err = std::current_exception();
        }
    };
    for (int t = 1; t < T; t++) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    if (err) std::rethrow_exception(err);
}

static const int kClsRows[4] = {48, 64, 96, 128};
static const int OBK = 4;   // 64-column blocks per outer (256-column) block of the panel factorisation
static const FrontArg kNoFront{0, 0, 0, 0, 0, 0, 0};

// The small fronts of a level (fused one-workgroup kernels) and its big fronts (assembly -> panel chain -> SYRK)
// only depend on the levels below, not on each other: when a level has both, the small ones run on the second
// stream next to the big-front pipeline, and the level ends when both have.
// A level with small fronts only still has up to four size classes = four launches with a tail each: the widest
// non-empty class stays on the main stream, the others go to the second one.
bool Device::factor_small_fronts(const LevelInfo &L) {
    const int nf = L.nbig();
    int ncls_used = 0, widest = -1;
    for (int k = 0; k < 4; k++) if (L.ncls[k] > 0) { ncls_used++; widest = k; }
    const bool split_small = L.nsmall > 0 && (nf > 0 || ncls_used > 1);
    if (split_small) {
        HC(hipEventRecord(ev_ready_, stream));
        HC(hipStreamWaitEvent(stream3, ev_ready_, 0));
    }
    for (int k = 0, off = 0; k < 4; off += L.ncls[k], k++) {
        hipStream_t st_small = !split_small ? stream : (nf > 0 || k != widest) ? stream3 : stream;
        launch_factor_small(st_small, ds_, d_levellist_ + L.first + off, L.ncls[k], kClsRows[k], nz_src_, d_L_, d_cb_, d_info_);
    }
    return split_small;
}

// One panel chain of a level: its stream and its fronts -- the level's width-sorted list of big fronts, or (two chains) the
// fronts at its even / odd positions, sorted as well.
struct Device::PanelChain {
    hipStream_t st;
    const FrontView *views;   // geometry records of the chain's fronts
    int half;                 // -1: the whole list, 0 / 1: its even / odd positions
    // geometry of the widest front of the chain: when it is the only one still active, the panel kernels get it in
    // their arguments (kernels.h, FrontArg)
    FrontArg f1;
    // of the first a fronts of the level's list, those on this chain
    int of(int a) const { return half < 0 ? a : half == 0 ? (a + 1) / 2 : a / 2; }
    // the chain's fronts with a 64-column block b: the first count(L, b) of views
    int count(const LevelInfo &L, int b) const { return of(L.wider_than(b * NB)); }
    const FrontArg &arg(int active) const { return active == 1 ? f1 : kNoFront; }
};

// Block b of a chain: potrf64 of the diagonal blocks -> trsm of the rows below -> the updates of the two-level blocking.
void Device::panel_block(const PanelChain &ch, const LevelInfo &L, int b) {
    const int n = ch.count(L, b), kb = b * NB;
    if (n <= 0) return;
    hipStream_t st = ch.st;
    const FrontView *hl = ch.views;
    if (b == 0 && n > 1) {
        // first block of a level with many fronts: one launch per width class (the list is sorted by decreasing width;
        // the even / odd halves of two chains are sorted as well), each in the workgroup shape that fits it
        const int cut[5] = {0, ch.of(L.wider[0]), ch.of(L.wider[1]), ch.of(L.wider[2]), n};
        const int wcls[4] = {64, 48, 32, 16};
        for (int q = 0; q < 4; q++)
            if (cut[q + 1] > cut[q])
                launch_potrf64(st, ds_, hl + cut[q], cut[q + 1] - cut[q], kb, d_L_, d_info_, kNoFront, std::min(wcls[q], L.max_cols));
    } else
        launch_potrf64(st, ds_, hl, n, kb, d_L_, d_info_, ch.arg(n), std::min(NB, L.max_cols - kb));
    {
        // first block of a level with many fronts: the fronts at most 32 columns wide (the tail of the sorted list) go to
        // the narrow-block kernel (same arithmetic on half the registers: more resident waves)
        constexpr int narrow_min = 256;
        const int cut32 = b == 0 ? ch.of(L.wider[1]) : n;
        const int nnarrow = n - cut32;
        if (b == 0 && narrow_min > 0 && nnarrow >= narrow_min) {
            if (cut32 > 0) launch_trsm(st, ds_, hl, cut32, kb, 0, L.max_rows - kb - 1, d_L_, nullptr, nullptr, kNoFront);
            launch_trsm_narrow(st, hl + cut32, nnarrow, kb, L.max_rows - kb - 1, d_L_);
        } else
            launch_trsm(st, ds_, hl, n, kb, 0, L.max_rows - kb - 1, d_L_, nullptr, nullptr, ch.arg(n));
    }
    // two-level blocking: K = 64 updates only inside the current 256-column block, the
    // rest of the panel once per block with K = 256
    const int J1 = (b / OBK + 1) * OBK;   // first 64-block of the next 256-column block
    const int nnext = ch.count(L, b + 1), nouter = ch.count(L, J1);     // (0 behind the widest front's last block)
    if (b + 1 < J1 && nnext > 0)
        launch_gemm_nt(st, ds_, hl, nnext, kb, NB, kb + NB, J1 * NB, L.max_rows - kb - NB,
                       std::min(J1 * NB, L.max_cols) - kb - NB, d_L_, ch.arg(nnext));
    if (b + 1 == J1 && nouter > 0)
        launch_gemm_nt(st, ds_, hl, nouter, (J1 - OBK) * NB, OBK * NB, J1 * NB, INT_MAX,
                       L.max_rows - J1 * NB, L.max_cols - J1 * NB, d_L_, ch.arg(nouter));
}

// The panel factorisation of a level is a chain of small dependent launches per 64-column block (potrf64 on ONE
// workgroup per front -> trsm -> gemm): while the diagonal blocks factor, the chip idles. Levels with several
// wide fronts run TWO independent chains -- the fronts at even / odd positions of the width-sorted list -- on two
// streams, so one half's trsm / gemm fills the chip while the other half sits in potrf64. Same arithmetic per
// front: bit-identical factor.
// (Measured and dropped -- DESIGN.md section 3: a look-ahead diagonal chain with the bulk one step behind on a second stream,
//  a persistent kernel per 256-column outer block, a pair chain, a rolling SYRK: the chain is bounded by the 64 x 64
//  factorisation and by single-CU tile rates, not by its dispatches.)
bool Device::factor_panel_chains(const LevelInfo &L) {
    const int nf = L.nbig(), nblk = L.nblk(), base = L.first + L.nsmall;
    const bool two = nf >= 2 && nblk >= 4 && !sharded();
    if (two) {
        HC(hipEventRecord(ev_ready2_, stream));               // (after the assembly of this level's panels)
        HC(hipStreamWaitEvent(stream3, ev_ready2_, 0));
    }
    auto front_at = [&](int pos) {       // position pos of the level's list of big fronts (kNoFront: the list is shorter)
        if (pos >= nf) return kNoFront;
        const i32 s = S_->levellist[base + pos];
        return FrontArg{1, (int)s, S_->ncols(s), S_->nrows(s), (int)S_->ld[s], (int)S_->sfirst[s], (long long)S_->panelptr[s]};
    };
    const PanelChain ch[2] = {{stream, two ? d_frec2_ + base : d_frec_ + base, two ? 0 : -1, front_at(0)},
                              {stream3, d_frec2_ + base + (nf + 1) / 2, 1, front_at(1)}};
    // (the two chains are enqueued block by block in turn, not one after the other: the host stays ahead of both)
    for (int b = 0; b < nblk; b++)
        for (int h = 0; h < (two ? 2 : 1); h++) panel_block(ch[h], L, b);
    if (two) {
        HC(hipEventRecord(ev_done1_, stream3));
        HC(hipStreamWaitEvent(stream, ev_done1_, 0));
    }
    return two;
}

// The contribution blocks of a level's big fronts (children gathered + L21 L21'). The level's launches read the device's wall
// clock themselves -- k_syrk_cb_rec per tile (reduced behind the last level, factor_levels), the others straight into slot `slot`
// of the stamps behind the pivot word (kernel_common.h, stamp_begin / stamp_end) --: earliest start, latest end over their
// workgroups, with nothing on the stream between the launches and their neighbours (syrk_ms()).
void Device::factor_contribution_blocks(const LevelInfo &L, int slot) {
    const int *list = d_levellist_ + L.first + L.nsmall;
    const int nf = L.nbig();
    unsigned long long *stamp = syrk_stamps(d_info_) + 2 * slot;
    unsigned long long *times = d_syrk_times_ + 2 * L.syrk_off;       // k_syrk_cb_rec: per tile; factor_levels reduces them into the slot
    // levels of HUGE fronts (3-D problems): the children's extend-add alone, then the product on 128 x 128 staged tiles
    const bool huge = env_.syrk_xcd && !sharded() && L.max_trail >= 4096 && L.max_cols >= 1024;
    // levels of wide fronts (the product dominates the tile): the software-pipelined product loop (factor_kernels.hip, k_syrk_cb_rec<true>;
    // same sums in the same order: a level's choice does not show in the bits)
    if (env_.syrk_xcd) launch_syrk_cb_recs(stream, ds_, d_syrk_recs_ + L.syrk_off, L.syrk_split, L.syrk_per, d_L_, d_cb_, times, huge ? 1 : 0, L.max_cols >= env_.syrk_piped_min);
    else launch_syrk_cb(stream, ds_, list, nf, L.max_trail, d_L_, d_cb_, stamp);
    if (huge) launch_syrk_big(stream, ds_, list, nf, L.max_trail, d_L_, d_cb_, stamp);       // (the slot spans both launches)
}

void Device::factor_levels(int lo, int hi, bool record_level_events) {
    if (lo == 0) {
        // the pivot word = "no failure", every SYRK slot = (start: all ones, end: 0), in one small launch
        launch_factor_reset(stream, d_info_, syrk_stamps(d_info_), S_->nlevels);
        syrk_launches = 0;
        // whole small subtrees first (one workgroup each), then the level schedule of everything above
        for (int k = 0, off = 0; k < 3; off += nsub_cls_[k], k++)
            launch_subtree(stream, ds_, 0, d_sub_first_ + off, d_sub_last_ + off, nsub_cls_[k], kClsRows[k], nz_src_, d_L_, d_cb_,
                           d_info_, nullptr, nullptr, 0, 0);
    }
    // Q's values in assembly order, on the second stream beside the first (small-front) levels; the first big-front assembly waits
    // for them. The gather stays PENDING (nzp_pending_) until some call has made the main stream wait for it: a later phase of a
    // sharded factorisation joins it before its first assembly if the phase that started it never did (no big front below the
    // shard level), and a call that started it and never needed it joins it before returning -- the kernel reads the CALLER's
    // values, which must not be in use once the call is over.
    if (lo == 0) {
        HC(hipEventRecord(ev_nzp0_, stream));
        HC(hipStreamWaitEvent(stream3, ev_nzp0_, 0));
        launch_gather_values(stream3, nz_src_, ds_.qsrc, d_nzp_, nq_);
        HC(hipEventRecord(ev_nzp_, stream3));
        nzp_pending_ = true;
    }
    int nsy = (int)syrk_launches;
    for (int lev = lo; lev < hi; lev++) {
        const LevelInfo &L = levels_[lev];
        if (env_.level_mark) { launch_level_mark(stream, 3, lev); level_event(stream, 0, lev); }
        const int nf = L.nbig();
        const bool split_small = factor_small_fronts(L);
        if (nf > 0 && nzp_pending_) { HC(hipStreamWaitEvent(stream, ev_nzp_, 0)); nzp_pending_ = false; }
        launch_assemble(stream, ds_, d_levellist_ + L.first + L.nsmall, d_arec_ + L.first + L.nsmall, d_nzp_, nf, L.max_cols, L.max_rows, nz_src_, d_L_, d_cb_);
        const bool two = factor_panel_chains(L);
        if (nf > 0 && L.max_trail > 0) factor_contribution_blocks(L, nsy++);
        if (split_small && !two) {        // (with two chains the join before the SYRK already covered the small fronts)
            HC(hipEventRecord(ev_done1_, stream3));
            HC(hipStreamWaitEvent(stream, ev_done1_, 0));
        }
        if (record_level_events) HC(hipEventRecord(ev_flevel_[lev], stream));      // the panels of this level are final: its sweep may start
    }
    // the tile times of the levels' SYRK launches into their slots: one launch behind the last level
    if (nsy > (int)syrk_launches && env_.syrk_xcd) launch_syrk_reduce(stream, d_syrk_level_times_ + lo, hi - lo, d_syrk_times_, syrk_stamps(d_info_));
    syrk_launches = nsy;
    if (lo == 0 && nzp_pending_) { HC(hipStreamWaitEvent(stream, ev_nzp_, 0)); nzp_pending_ = false; }     // (see above)
    if (env_.level_mark) level_event(stream, 0, hi);
}

// The dense inverses are only needed by the sweeps and the selected inversion of the big
// fronts, never by logdet: they are computed lazily (first solve / selinv after a
// refactorisation) on a side stream, so that in a refactorise+solve step they overlap the
// small-front levels at the bottom of the forward sweep.
void Device::start_inverse_async() {
    if (!inverse_pending) return;
    // ev_fact_ = "the factor is final": recorded at the end of the factorisation, so that whatever the caller has put on
    // the main stream since then (the transpose of the right-hand sides) does not hold the inverses back
    if (!fact_event_valid_) HC(hipEventRecord(ev_fact_, stream));
    fact_event_valid_ = false;
    HC(hipStreamWaitEvent(stream2, ev_fact_, 0));
    invert_diag_blocks(stream2, NB, inv_cap_);
    HC(hipEventRecord(ev_inv_, stream2));
    inverse_pending = false;
    inverse_full_ = inv_maxc_ <= inv_cap_;
}
void Device::wait_inverse(hipStream_t st) { HC(hipStreamWaitEvent(st, ev_inv_, 0)); }

// Called behind the synchronisation of a factorisation, before anything reads the inverses (see device.h).
void Device::decide_inverse_cap() {
    if (inv_cap_decided_ || sharded() || *h_info_ != INT_MAX) return;     // a failed pivot: the next good factorisation decides
    inv_cap_decided_ = true;
    const int nf = inv_nact_.empty() ? 0 : inv_nact_[0];                   // the fronts wider than NB
    if (nf <= 0 || inv_cap_ <= NB) return;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t cnt = (size_t)nf * (size_t)((inv_maxc_ + 255) / 256);     // partial maxima: row blocks x fronts
    if (!d_pivgrowth_) d_pivgrowth_ = dalloc<double>(cnt);
    launch_pivot_growth(stream, ds_, d_invlist_, nf, inv_maxc_, d_L_, d_pivgrowth_);
    std::vector<double> r(cnt);
    HC(hipMemcpyAsync(r.data(), d_pivgrowth_, cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    ms_inv_decide = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (double v : r)
        if (!(v <= kInvGrowthMax)) {
            inv_cap_ = NB;
            break;
        }
}

void Device::invert_diag_blocks(hipStream_t stream, int b_from, int b_to) {
    int stage = 0;
    for (int B = NB; B < std::min(inv_maxc_, b_to); B *= 2, stage++) {
        if (B < b_from) continue;
        const int na = inv_nact_[stage];
        if (na <= 0) break;
        launch_inv_stage(stream, ds_, d_invlist_, na, B, inv_maxc_, 1, d_L_, d_invT_, d_inv_toff_[stage]);
        launch_inv_stage(stream, ds_, d_invlist_, na, B, inv_maxc_, 2, d_L_, d_invT_, d_inv_toff_[stage]);
    }
}

void Device::invert_level(hipStream_t st, int lev) {
    if (inv_lvl_first_.empty() || inv_lvl_maxc_[lev] <= NB) return;
    int stage = 0;
    for (int B = NB; B < std::min(inv_lvl_maxc_[lev], inv_cap_); B *= 2, stage++) {
        const int na = inv_lvl_nact_[lev][stage];
        if (na <= 0) break;
        launch_inv_stage(st, ds_, d_inv_lvl_list_ + inv_lvl_first_[lev], na, B, inv_lvl_maxc_[lev], 1, d_L_, d_invT_, d_inv_lvl_toff_[stage] + inv_lvl_first_[lev]);
        launch_inv_stage(st, ds_, d_inv_lvl_list_ + inv_lvl_first_[lev], na, B, inv_lvl_maxc_[lev], 2, d_L_, d_invT_, d_inv_lvl_toff_[stage] + inv_lvl_first_[lev]);
    }
}

// Numeric factorisation + solve in ONE call, pipelined (gmrfx_refactorize_solve; the reference does both inside one call as
// well: workspace_solve = ensure_numeric! -> refactorize!, then backend_solve, src/workspace/gmrf_workspace.jl:170-178, 207-215).
// The top of the factorisation is a chain of small dependent launches that leaves most of the chip idle, the bottom of the
// forward sweep is throughput work that only needs the BOTTOM of the factor: the forward sweep (transpose in, sweep tasks,
// then level by level: dense-inverse stages of the level, assembly, triangular product, update) runs on the low-priority
// side stream and follows the factorisation up the tree -- level l starts when the event "level l is factored" has passed.
// When the root has been factored only the root's own forward step is left; the backward sweep follows on the main stream.
// Same kernels, same operands, same order per front as refactorize() + solve(): bit-identical results.
void Device::refactorize_solve(const double *nzval, bool nz_on_device, const double *B, long long ldb, long long nrhs, double *X, long long ldx_out,
                               bool b_on_device) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("sharded handle: use the phase entry points (gmrfx/shard.py)");
    // nothing to pipeline / the caller's stream / the inverse cap is not decided yet (the handle's first factorisation): the plain
    // sequence
    if (nrhs <= 0 || stream != own_stream_ || !inv_cap_decided_) {
        refactorize(nzval, nz_on_device);
        if (nrhs > 0) solve(B, ldb, nrhs, X, ldx_out, b_on_device, 0);
        return;
    }
    const long long n = S_->n;
    const int nl = (int)levels_.size();
    const double *src = nzval;
    if (!nz_on_device) {
        host_upload_values(nzval);
        src = d_nz_;
    }
    ensure_rhs_capacity(nrhs);
    const double *dB = B;
    double *dXo = X;
    long long ldin = ldb, ldout = ldx_out;
    if (!b_on_device) {
        ensure_io(n * nrhs);
        dB = d_io_; dXo = d_io_; ldin = n; ldout = n;
    }
    while ((int)ev_flevel_.size() < nl + 1) { Event e; e.create(hipEventDisableTiming); ev_flevel_.push_back(std::move(e)); }
    // host right-hand sides: in FRONT of the factorisation (see the measurements above host_upload): the transfers are serial --
    // B in, the pipelined step, X out -- never beside the factorisation
    if (!b_on_device) {
        host_upload(B, ldb, nrhs, d_io_);
        HC(hipStreamWaitEvent(stream, ev_up_, 0));
    }
    begin_factor(src);
    HC(hipEventRecord(ev_ready_, stream));                 // the side stream starts behind the uploads / whatever precedes this call
    factor_levels(0, nl, true);
    enqueue_factor_tail();
    // ---- first pass (pass_width(): up to 64 columns -- the width solve() uses, so that the two forms of the step give the
    // same bits): forward sweep on the side stream, behind the level events
    const int PW = pass_width(nrhs);
    const int nr = (int)std::min<long long>(PW, nrhs), ldx = nr;
    const Event *ev = ev_lane_[0];
    // lane 0's buffers on the side stream for the forward half, on the main stream for the rest
    const SweepLane ln0 = lane(0), side{stream2, ln0.X, ln0.X2, ln0.W};
    HC(hipStreamWaitEvent(side.st, ev_ready_, 0));
    if (!b_on_device) HC(hipStreamWaitEvent(side.st, ev_up_, 0));
    HC(hipEventRecord(ev[0], side.st));
    launch_permute(side.st, d_iperm_, (int)n, const_cast<double *>(dB), ldin, side.X, nr, ldx, 0);
    HC(hipEventRecord(ev[1], side.st));
    forward(side, nr, ldx, 0, nl, true);
    HC(hipEventRecord(ev_inv_, side.st));                // every level's inverses exist: later solves pass wait_inverse() at once
    HC(hipEventRecord(ev[2], side.st));
    inverse_pending = false;
    inverse_full_ = inv_maxc_ <= inv_cap_;
    enqueue_logdet(stream2, false);                     // behind the forward sweep on the side stream: beside the backward sweep
    HC(hipStreamWaitEvent(stream, ev[2], 0));
    backward(ln0, nr, ldx, true, nl, 0);
    HC(hipEventRecord(ev[3], stream));
    launch_permute(stream, d_iperm_, (int)n, dXo, ldout, ln0.X, nr, ldx, 1);
    HC(hipEventRecord(ev[4], stream));
    // ---- further passes: the factor is complete, plain sweeps on the main stream (no per-pass events)
    for (long long j0 = PW; j0 < nrhs; j0 += PW)
        sweep_pass(ln0, nullptr, dB + j0 * ldin, ldin, dXo + j0 * ldout, ldout, (int)std::min<long long>(PW, nrhs - j0), 0, nullptr);
    HC(hipEventRecord(ev_lane_[1][0], stream));
    if (!b_on_device) host_download(d_io_, nrhs, X, ldx_out, stream);
    HC(hipStreamSynchronize(stream));
    finish_factor();                                    // (the inverse cap was decided before this call could be taken)
    float a = 0, b = 0, c = 0, d = 0, tail = 0;
    HC(hipEventElapsedTime(&a, ev[0], ev[1]));
    HC(hipEventElapsedTime(&b, ev_[1], ev[2]));          // what is left of the forward sweep once the factor is complete
    HC(hipEventElapsedTime(&c, ev[2], ev[3]));
    HC(hipEventElapsedTime(&d, ev[3], ev[4]));
    HC(hipEventElapsedTime(&tail, ev_[1], ev_lane_[1][0]));
    ms_perm = a + d; ms_fwd = std::max(b, 0.0f); ms_bwd = b >= 0 ? c : c + b;
    ms_solve = tail;                                     // device time behind the factorisation: ms_factor + ms_solve = the step
    last_nrhs = nrhs;
}

// ---- what every numeric factorisation of an unsharded handle shares (refactorize, refactorize_solve, refactorize_logpdf,
// batch_refactorize_logpdf): begin_factor -> factor_levels -> enqueue_factor_tail -> [whatever else the call enqueues] -> the
// call's ONE synchronisation -> finish_factor. The caller says what becomes of the dense inverses (inverse_pending, or complete).
// d_src: Q's values on the device (d_nz_ or the caller's buffer). A caller's buffer is read in place (the Q scatter happens
// inside the assembly kernels, and the call only returns once they have finished): no private copy.
void Device::begin_factor(const double *d_src) {
    nz_src_ = d_src;
    nz_held_ = (d_src == d_nz_);
    factor_serial_++;
    HC(hipEventRecord(ev_[0], stream));
}
// behind the last level: the timing / "factor is final" events, and the pivot report on its way to the pinned host word (it
// travels with the factorisation: no blocking copy after the synchronisation)
void Device::enqueue_factor_tail() {
    HC(hipEventRecord(ev_[1], stream));
    HC(hipEventRecord(ev_fact_, stream));
    fact_event_valid_ = true;
    HC(hipMemcpyAsync(h_info_, d_info_, info_bytes(syrk_launches), hipMemcpyDeviceToHost, stream));     // (the SYRK stamps ride along)
}
// behind the synchronisation. `factorized` is set HERE for every caller, once the synchronisation has succeeded: a call that
// throws on the way leaves the handle as it found it. (decide_inverse_cap returns at once when the cap is decided -- always so in
// the pipelined call.)
void Device::finish_factor() {
    info_cached_ = true;
    HC(hipGetLastError());
    decide_inverse_cap();
    float ms = 0;
    HC(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
    ms_factor = ms;
    syrk_times_pending_ = true;      // the per-launch stamps are only summed when somebody asks for the statistics
    factorized = true;
    selinv_valid = false;
}

void Device::refactorize(const double *nzval, bool on_device) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("sharded handle: use gmrfx_refactorize_phase (two phases with an exchange in between)");
    const double *src = nzval;
    if (!on_device) {
        HC(hipMemcpyAsync(d_nz_, nzval, (size_t)S_->nnz_in * sizeof(double), hipMemcpyHostToDevice, stream));
        src = d_nz_;
    }
    begin_factor(src);
    factor_levels(0, (int)levels_.size(), false);
    enqueue_factor_tail();
    inverse_pending = true;
    HC(hipStreamSynchronize(stream));
    finish_factor();
}

void Device::refactorize_phase(const double *d_nzval, int phase) {
    HC(hipSetDevice(device));
    if (!sharded()) throw std::invalid_argument("gmrfx_refactorize_phase needs a sharded handle (shard_world > 1, or shard_min_top > 0)");
    const int nl = (int)levels_.size();
    const int split = std::min<int>(S_->shard_level, nl);
    info_cached_ = false;
    fact_event_valid_ = false;
    factor_serial_++;
    HC(hipEventRecord(ev_[0], stream));
    if (phase == 0) {               // the subtrees this rank owns
        nz_src_ = d_nzval;
        nz_held_ = false;       // the values live in the caller's device buffer
        factorized = false;
        factor_levels(0, split, false);
    } else {                        // top level split + phase - 1: the fronts of that level this rank owns
        const int lev = split + phase - 1;
        if (lev >= nl) throw std::invalid_argument("refactorize phase beyond the last level");
        factor_levels(lev, lev + 1, false);
    }
    syrk_times_pending_ = true;      // (the slots accumulate over the phases as syrk_launches does; syrk_ms() fetches them)
    HC(hipEventRecord(ev_[1], stream));
    if (!async_phases_) {
        HC(hipStreamSynchronize(stream));
        HC(hipGetLastError());
        float ms = 0;
        HC(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
        ms_factor = phase == 0 ? ms : ms_factor + ms;
    }
    selinv_begun_ = false;
    if (split + phase >= nl) { factorized = true; selinv_valid = false; inverse_pending = true; }   // last phase done
}

// Distributed top fronts (symbolic.h): block phases of one front's factorisation, driven by gmrfx/shard.py between the
// broadcasts. 256-column blocks dealt cyclically over the front's group; the same kernels and the same sums in the same order
// as the level loop uses for a front of its own (potrf64 -> trsm -> K = 64 update inside the block; K = 256 update of the later
// blocks; children gathered + L21 L21' per 64 x 64 tile of the contribution block), so the factor equals the unsharded one.
void Device::dist_front_phase(const double *d_nzval, int front, int what, int block) {
    HC(hipSetDevice(device));
    if (front < 0 || front >= S_->nsuper || !S_->is_dist(front)) throw std::invalid_argument("not a distributed front of this handle");
    const i32 R = front;
    const int g = S_->group_size(R), me = S_->group_pos(R, S_->shard_rank);
    if (me < 0) return;
    const int c = S_->ncols(R), r = S_->nrows(R);
    const int nob = S_->panel_blocks(R);
    const FrontArg fa{1, (int)R, c, r, (int)S_->ld[R], (int)S_->sfirst[R], (long long)S_->panelptr[R]};
    // Block-cyclic STORAGE (Symbolic::compact_here: a front without trailing rows on a member that is not its owner): this rank holds
    // its own blocks one behind the other + a window of two received blocks. The kernels keep addressing columns globally: block b is
    // handed to them under the pseudo panel base that puts its columns where they are stored, and the K operand of a panel update
    // (the block column just received, or an own one) under a base of its own (FrontArg::ppa).
    const bool compact = S_->compact_here(R);
    const long long ldR = S_->ld[R], ppl = S_->panelptr[R];
    auto blk_pp = [&](int b) -> long long { return compact ? ppl - 256LL * (b - b / g) * ldR : ppl; };
    auto a_pp = [&](int b) -> long long {
        if (!compact) return kNoPpa;
        return b % g == me ? blk_pp(b) : ppl + S_->compact_window(R, b & 1) - 256LL * b * ldR;
    };
    if (!d_dist_list_) {
        d_dist_list_ = dalloc<int>(S_->dist_fronts.size());
        HC(hipMemcpyAsync(d_dist_list_, S_->dist_fronts.data(), S_->dist_fronts.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    }
    const int *list = d_dist_list_ + S_->dist_index[R];
    if (what == 0) {
        if (!d_nzval) throw std::invalid_argument("d_nzval is null");
        launch_assemble_cyclic(stream, ds_, list, c, d_nzval, d_L_, d_cb_, g, me, compact);
    } else if (what == 1) {
        if (block < 0 || block >= nob) throw std::invalid_argument("distributed front: block out of range");
        if (block % g != me) return;
        FrontArg fb = fa;
        fb.pp = blk_pp(block);
        const int b0 = block * OBK, b1 = std::min(b0 + OBK, (c + NB - 1) / NB);
        for (int b = b0; b < b1; b++) {
            const int kb = b * NB;
            launch_potrf64(stream, ds_, nullptr, 1, kb, d_L_, d_info_, fb);
            launch_trsm(stream, ds_, nullptr, 1, kb, 0, r - kb - 1, d_L_, nullptr, nullptr, fb);
            if (b + 1 < b1)
                launch_gemm_nt(stream, ds_, nullptr, 1, kb, NB, kb + NB, b1 * NB, r - kb - NB, std::min(b1 * NB, c) - kb - NB, d_L_, fb);
        }
    } else if (what == 2 || what == 4 || what == 5) {
        // 2: block -> all my later blocks; 4: -> block + 1 only (look-ahead: its owner factors and broadcasts it next, while
        // everybody applies `block` to the rest); 5: -> my later blocks except block + 1. 4 then 5 = 2: same sums, same order per entry.
        if (block < 0 || block >= nob) throw std::invalid_argument("distributed front: block out of range");
        const int k0 = block * 256, K = std::min(256, c - k0);
        const int jlo = what == 5 ? block + 2 : block + 1, jhi = what == 4 ? std::min(block + 2, nob) : nob;
        for (int j = jlo; j < jhi; j++) {
            if (j % g != me) continue;
            const int c0 = j * 256;
            FrontArg fj = fa;
            fj.pp = blk_pp(j);
            fj.ppa = a_pp(block);
            launch_gemm_nt(stream, ds_, nullptr, 1, k0, K, c0, c0 + 256, r - c0, std::min(256, c - c0), d_L_, fj);
        }
    } else if (what == 3) {
        if (r > c) launch_syrk_cb_cyclic(stream, ds_, list, r - c, d_L_, d_cb_, g, me, nob);
    } else throw std::invalid_argument("distributed front phase must be 0 (assemble), 1 (factor block), 2 / 4 / 5 (apply block: all / next / rest) or 3 (contribution block)");
    if (!async_phases_) HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

void Device::set_prior(const double *prior_nzval, const long long *map, long long cnt) {
    HC(hipSetDevice(device));
    const long long nnz = S_->nnz_in;
    for (long long k = 0; k < cnt; k++)
        if (map[k] < 0 || map[k] >= nnz) throw std::invalid_argument("Hessian index map points outside the stored pattern of Q");
    if (!d_prior_) d_prior_ = dalloc<double>((size_t)nnz);
    HC(hipMemcpyAsync(d_prior_, prior_nzval, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, stream));
    if (cnt > hmap_cap_ || !d_hmap_ || !d_h_) {
        hmap_cap_ = 0;      // (if the second allocation throws, the next call regrows both)
        regrow(d_hmap_, (size_t)cnt, &bytes_total);
        regrow(d_h_, (size_t)cnt, &bytes_total);
        hmap_cap_ = cnt;
    }
    hmap_cnt_ = cnt;
    h_hmap_.assign(map, map + cnt);
    prior_diag_ = -1;
    prior_design_ = -1;
    bprior_design_ = false;      // (bset_prior says otherwise)
    bprior_map_ok_ = -1;
    if (cnt > 0) HC(hipMemcpyAsync(d_hmap_, map, (size_t)cnt * sizeof(long long), hipMemcpyHostToDevice, stream));
    HC(hipStreamSynchronize(stream));
}
// the Hessian values to the device (when they are the host's), then d_nz_ = prior, d_nz_[map[k]] -= h[k]
void Device::newton_values(const double *h, bool on_device) {
    if (!d_prior_) throw std::invalid_argument("gmrfx_set_prior has not been called");
    const double *dh = h;
    if (!on_device && hmap_cnt_ > 0) {
        HC(hipMemcpyAsync(d_h_, h, (size_t)hmap_cnt_ * sizeof(double), hipMemcpyHostToDevice, stream));
        dh = d_h_;
    }
    launch_newton_update(stream, d_prior_, d_nz_, S_->nnz_in, d_hmap_, dh, hmap_cnt_);
}
void Device::refactorize_update(const double *h, bool on_device) {
    HC(hipSetDevice(device));
    newton_values(h, on_device);
    refactorize(d_nz_, true);
}

// One Newton iterate as one pipelined call: Q_k = Q_prior - H_k on the device, numeric factorisation, solve
// (gaussian_approximation.jl:103-129: _update_hessian!, ensure_numeric!, then the solve for the new mean)
void Device::refactorize_update_solve(const double *h, bool h_on_device, const double *B, long long ldb, long long nrhs, double *X, long long ldx,
                                      bool b_on_device) {
    HC(hipSetDevice(device));
    newton_values(h, h_on_device);
    refactorize_solve(d_nz_, true, B, ldb, nrhs, X, ldx, b_on_device);
}

double Device::syrk_ms() {
    if (syrk_times_pending_) {
        HC(hipSetDevice(device));
        if (!info_cached_ && syrk_launches > 0) {
            // (the phases of a sharded factorisation leave the stamps on the device; asynchronous phases / an external main
            //  stream: the factorisation may still run)
            HC(hipStreamSynchronize(stream));
            HC(hipMemcpy(syrk_stamps(h_info_), syrk_stamps(d_info_), info_bytes(syrk_launches) - info_bytes(0), hipMemcpyDeviceToHost));
        }
        const unsigned long long *stamp = syrk_stamps(h_info_);
        unsigned long long ticks = 0;
        for (long long k = 0; k < syrk_launches; k++)
            if (stamp[2 * k + 1] > stamp[2 * k]) ticks += stamp[2 * k + 1] - stamp[2 * k];       // (a slot nobody stamped: start all ones, end 0)
        ms_syrk = (double)ticks / wall_clock_khz_;
        syrk_times_pending_ = false;
    }
    return ms_syrk;
}

long long Device::fail_col() {
    int v = INT_MAX;
    if (info_cached_) v = *h_info_;
    else {
        HC(hipStreamSynchronize(stream));       // (asynchronous phases / an external main stream: the factorisation may still run)
        HC(hipMemcpy(&v, d_info_, sizeof(int), hipMemcpyDeviceToHost));
    }
    return v == INT_MAX ? -1 : v;
}

void Device::ensure_rhs_capacity(long long nrhs) {
    const long long chunk = std::min<long long>(nrhs, 64);
    if (chunk > rhs_cap_) {
        // (old buffers stay in allocs_ until destruction; capacity only ever grows to 64)
        d_X_ = dalloc<double>((size_t)S_->n * 64);
        d_X2_ = dalloc<double>((size_t)S_->n * 64);
        d_W_ = dalloc<double>((size_t)std::max<long long>(sum_trail_, 1) * 64);
        rhs_cap_ = 64;
    }
    if (pass_width(nrhs) < nrhs && !d_Xb_ && !sharded()) {
        d_Xb_ = dalloc<double>((size_t)S_->n * 64);
        d_X2b_ = dalloc<double>((size_t)S_->n * 64);
        d_Wb_ = dalloc<double>((size_t)std::max<long long>(sum_trail_, 1) * 64);
    }
}

// the staging buffer of host right-hand sides (solve, refactorize_solve): grown geometrically
void Device::ensure_io(long long need) {
    if (need <= io_cap_) return;
    const long long cap = std::max(need, 2 * io_cap_);
    regrow(d_io_, (size_t)cap, &bytes_total);
    io_cap_ = cap;
}

// The bottom subtrees. Up to env_.wave_max_nr (16) right-hand sides: one wave per (task, 16 columns), sweep_wave.hip, biggest LDS
// class first; wider passes: the chunk form, four waves per (task, 16 columns), sweep_chunk.hip. Measured at cfg 2, round 5
// (tools/nrhs_sweep.py, ms per solve, wave form / chunk form): 1 RHS 2.88 / 3.22, 16: 3.00 / 3.36, 32: 3.71 / 3.47, 64: - / 3.90 at the
// time of the choice; with the narrow level kernels and the local vector as wide as the pass: 1 RHS 1.65, 16: 2.28.
// GMRFX_TASK_MODE = wg / wave forces one form.
void Device::sweep_tasks(const SweepLane &ln, int phase, int nr, int ldx, bool follows_factor) {
    if (nr > env_.wave_max_nr) {
        // pipelined call: the forward task kernel runs beside the top of the factorisation -- TWO resident workgroups per CU
        // instead of four (16 KB of unused dynamic LDS on top of its 40 KB), so that the panel chain's kernels find LDS
        // (measured at cfg 2, round 5: pad 0 / 8 / 16 / 42 KB -> step 12.59 / 12.61 / 12.38 / 12.91 ms)
        constexpr int pad_kb = 16;
        const size_t extra = (follows_factor && phase == 1) ? (size_t)pad_kb * 1024 : 0;
        ensure_dtile(ln.st);
        launch_sweep_chunks(ln.st, ds_, phase, d_swt_, nswt_, d_swc_fwd_, d_swc_bwd_, d_swc_listf_, d_swc_listb_, d_dtile_, d_L_, ln.X,
                            phase == 1 ? ln.W : nullptr, nr, ldx, extra);
        return;
    }
    ensure_rdiag(ln.st);
    if (nr <= 4) {      // the local vector of such a pass is 9 KB at most whatever the class: one launch, no tail of the big class before the small one starts
        launch_wave_tasks(ln.st, ds_, phase, d_swt_, d_wave_order_ + nswt_, nswt_, kWaveRows[kWaveClasses - 1], d_L_, d_rdiag_, d_rdiag_ + S_->n, ln.X,
                          ln.W, nr, ldx);
        return;
    }
    for (int k = kWaveClasses - 1; k >= 0; k--)
        launch_wave_tasks(ln.st, ds_, phase, d_swt_, d_wave_order_ + wave_first_[k], wave_count_[k], kWaveRows[k], d_L_, d_rdiag_,
                          d_rdiag_ + S_->n, ln.X, ln.W, nr, ldx);
}

// 1 / L_jj (+ the zero word masked operand elements are read from), once per factorisation, on stream st:
// solve() calls this on the main stream BEFORE its lanes fork, so that a second lane never reads it half-written
void Device::ensure_rdiag(hipStream_t st) {
    if (env_.wave_max_nr <= 0 || nswt_ <= 0) return;
    if (!d_rdiag_) { d_rdiag_ = dalloc<double>((size_t)S_->n + 2); rdiag_for_ = 0; }
    if (rdiag_for_ == factor_serial_) return;
    launch_rdiag(st, d_L_, ds_.diagoff, (int)S_->n, d_rdiag_);
    HC(hipMemsetAsync(d_rdiag_ + S_->n, 0, 2 * sizeof(double), st));
    rdiag_for_ = factor_serial_;
}

// the chunks' inverse diagonal blocks in MFMA operand order, once per factorisation, on stream st (solve() calls this on the
// main stream BEFORE its lanes fork; the pipelined call on the side stream behind the gate event, when the task fronts are final)
void Device::ensure_dtile(hipStream_t st) {
    if (nswc_ <= 0 || dtile_for_ == factor_serial_) return;
    launch_pack_diag(st, d_swc_bwd_, nswc_, d_L_, d_dtile_);      // (the backward records hold every chunk once)
    dtile_for_ = factor_serial_;
}

SweepKnobs Device::sweep_knobs() const {
    return SweepKnobs{inv_cap_, env_.fwd_front_min, env_.bwd_front_min, env_.syrk_xcd, kNarrowPassMax, kNarrowPassMaxBwd,
                      kFrontMaxCols, kWaveSplitCols, kWaveSplitRows};
}

void Device::forward(const SweepLane &ln, int nr, int ldx, int lo, int hi, bool follows_factor) {
    const SweepKnobs knobs = sweep_knobs();
    if (env_.level_mark && lo == 0) { launch_level_mark(ln.st, 1, -1); level_event(ln.st, 1, 0); }
    // pipelined factor + solve (refactorize_solve): the bottom waits for the highest level a task / subtree reaches, every level
    // above for its own "factored" event; the dense inverses are built level by level instead of all at once
    if (follows_factor) {
        HC(hipStreamWaitEvent(ln.st, ev_flevel_[fused_gate_level_], 0));
        if (nr <= env_.wave_max_nr && nswt_ > 0) rdiag_for_ = 0;      // 1 / L_jj of the task fronts: their diagonals are final now, the rest is never read
        dtile_for_ = 0;                                            // (the same for the chunks' inverse diagonal blocks)
    }
    if (lo == 0) sweep_tasks(ln, 1, nr, ldx, follows_factor);
    if (lo == 0)
        for (int k = 0, off = 0; k < 3; off += nsub_cls_[k], k++)
            launch_subtree(ln.st, ds_, 1, d_sub_first_ + off, d_sub_last_ + off, nsub_cls_[k], kClsRows[k], nullptr, d_L_, nullptr,
                           nullptr, ln.X, ln.W, nr, ldx);
    for (int lev = lo; lev < hi; lev++) {
        const LevelInfo &L = swlevels_[lev];
        if (env_.level_mark) { launch_level_mark(ln.st, 1, lev); level_event(ln.st, 1, 1 + lev); }
        if (follows_factor) {
            if (lev > fused_gate_level_) HC(hipStreamWaitEvent(ln.st, ev_flevel_[lev], 0));
            invert_level(ln.st, lev);
        } else if (lev == std::max(lo, first_multiblock_level_)) wait_inverse(ln.st);
        for (int k = 0, off = 0; k < 4; off += L.ncls[k], k++)
            launch_fwd_small(ln.st, ds_, d_sw_levellist_ + L.first + off, L.ncls[k], kClsRows[k], d_L_, ln.X, ln.W, nr, ldx);
        const int *list = d_sw_levellist_ + L.first + L.nsmall;
        const FwdLevelPlan p = plan_forward_level(L, nr, knobs);
        // fronts of at most 128 columns (the tail of the list: sorted by decreasing width): the WHOLE step -- own rows assembled,
        // y = L11^-1 b, W = children - L21 y -- as one workgroup and one launch (k_fwd_front, sweep_front.hip), on levels with enough
        // of them to fill the chip and for passes wider than the narrow kernels take; wider fronts keep the three launches below
        if (p.ntail > 0) {
            launch_fwd_front(ln.st, ds_, list + p.nf, p.ntail, d_L_, ln.X, ln.X2, ln.W, nr, ldx);
            if (p.nf == 0) continue;
        }
        launch_fwd_assemble(ln.st, ds_, list, p.nf, L.max_cols, ln.X, ln.W, nr, ldx);   // own rows only
        // y = L11^-1 b as one triangular product per front (dense inverse, inverse.hip), then the
        // trailing update W -= L21 y with K = all columns of the front
        // y of the big fronts stays in X2 (no copy back): the update below and the backward sweep read it there
        // fronts wider than inv_cap_: block by block (y_j = X_jj b_j, then the own rows below -= L[.., block j] y_j)
        for (int j = 0; j < p.nbk; j++) {
            launch_xmul(ln.st, ds_, list, p.xmul_fronts(j), L.max_cols, 0, d_L_, ln.X, ln.X2, nr, ldx, j, inv_cap_);
            if (j + 1 < p.nbk) launch_fwd_own_update(ln.st, ds_, list, p.own_fronts(j), L.max_cols, d_L_, ln.X2, ln.X, nr, ldx, j, inv_cap_);
        }
        // W -= L21 y: the wave kernel for the fronts up to p.cmin columns wide (narrow passes), the split-K kernels for the wider ones
        if (p.wave) launch_fwd_update_wave(ln.st, ds_, d_fwd_recs_ + L.fwd_off, L.fwd_split, L.fwd_per, d_L_, ln.X2, ln.W, nr, ldx, p.cmin, p.wave_split_k);
        if (p.update == FwdLevelPlan::kRecords)
            launch_fwd_update_recs(ln.st, ds_, d_fwd_recs_ + L.fwd_off, L.fwd_split, L.fwd_per, d_L_, ln.X2, ln.W, nr, ldx, p.cmin);
        else if (p.update == FwdLevelPlan::kGrid)
            launch_fwd_update(ln.st, ds_, list, p.nf, L.max_trail, d_L_, ln.X2, ln.W, nr, ldx, p.cmin);
    }
    if (env_.level_mark) level_event(ln.st, 1, 1 + hi);
}

// y_in_x2: the forward sweep left y of the big fronts in X2 (full solve). The backward sweep then turns it
// into t = y - L21' x in place there and writes x = L11^-T t straight into X -- no copies. A backward-only
// solve (F.UP \ z) gets z in X: classic path with one copy per level.
void Device::backward(const SweepLane &ln, int nr, int ldx, bool y_in_x2, int hi, int lo) {
    const SweepKnobs knobs = sweep_knobs();
    // t lives where y was left (Xt), x = L11^-T t goes to the other buffer (Xx): X2 -> X after a forward sweep, X -> X2 in place
    double *const Xt = y_in_x2 ? ln.X2 : ln.X, *const Xx = y_in_x2 ? ln.X : ln.X2;
    wait_inverse(ln.st);   // (a no-op event wait once the forward sweep has passed it)
    for (int l = hi - 1; l >= lo; l--) {
        const LevelInfo &L = swlevels_[l];
        if (env_.level_mark) { launch_level_mark(ln.st, 2, l); level_event(ln.st, 2, (int)levels_.size() - 1 - l); }
        const int *list = d_sw_levellist_ + L.first + L.nsmall;
        for (int k = 0, off = 0; k < 4; off += L.ncls[k], k++)
            launch_bwd_small(ln.st, ds_, d_sw_levellist_ + L.first + off, L.ncls[k], kClsRows[k], d_L_, ln.X, nr, ldx);
        const BwdLevelPlan p = plan_backward_level(L, nr, knobs);
        // fronts of at most 128 columns (the tail of the list: sorted by decreasing width): the whole step as one workgroup and
        // one launch (sweep_front.hip); in place when y sits in X (own rows are read and written by their front alone)
        // Only on levels with enough such fronts to fill the chip: a workgroup walks its front's trailing rows batch after batch,
        // and a level of a hundred fronts with 700 trailing rows each is faster as many small workgroups (the two launches).
        if (p.ntail > 0) {
            launch_bwd_front(ln.st, ds_, list + p.nf, p.ntail, d_L_, ln.X, Xt, ln.X, nr, ldx);
            if (p.nf == 0) continue;
        }
        // t = y - L21' x: the wave kernel for the fronts with at most p.mmin trailing rows (narrow passes), the split-K kernels for the others
        if (p.wave) launch_bwd_wave(ln.st, ds_, list, p.nf, L.max_cols, d_L_, ln.X, Xt, nr, ldx, p.mmin, p.wave_split_k);
        if (p.gemm) launch_bwd_gemm(ln.st, ds_, list, p.nf, L.max_cols, d_L_, ln.X, Xt, nr, ldx, -1, 1 << 30, p.mmin);
        // fronts wider than inv_cap_: from the last block up, t_j -= L[own rows below, block j]' x, x_j = X_jj' t_j
        for (int j = p.nbk - 1; j >= 0; j--) {
            if (j + 1 < p.nbk) launch_bwd_gemm(ln.st, ds_, list, p.own_fronts(j), L.max_cols, d_L_, ln.X, Xt, nr, ldx, j, inv_cap_);
            launch_xmul(ln.st, ds_, list, p.xmul_fronts(j), L.max_cols, 1, d_L_, Xt, Xx, nr, ldx, j, inv_cap_);
            // in place: x_j has to be back in X before the block above reads it
            if (!y_in_x2) launch_copy_own(ln.st, ds_, list, p.xmul_fronts(j), L.max_cols, ln.X2, ln.X, nr, ldx, j, inv_cap_);
        }
    }
    if (env_.level_mark && lo == 0) { launch_level_mark(ln.st, 2, -1); level_event(ln.st, 2, (int)levels_.size()); }
    if (lo == 0)
        for (int k = 0, off = 0; k < 3; off += nsub_cls_[k], k++)
            launch_subtree(ln.st, ds_, 2, d_sub_first_ + off, d_sub_last_ + off, nsub_cls_[k], kClsRows[k], nullptr, d_L_, nullptr,
                           nullptr, ln.X, nullptr, nr, ldx);
    if (lo == 0) sweep_tasks(ln, 2, nr, ldx, false);
    if (env_.level_mark && lo == 0) level_event(ln.st, 2, (int)levels_.size() + 1);
}

// GMRFX_LEVEL_MARK=1: HIP events at the level boundaries of the most recent factorisation / forward / backward sweep
// (slot numbering in level_times()); a profiling aid behind gmrfx_level_times, never on in production runs
void Device::level_event(hipStream_t st, int phase, int slot) {
    auto &v = ev_level_[phase];
    while ((int)v.size() <= slot) { Event e; e.create(); v.push_back(std::move(e)); }
    HC(hipEventRecord(v[slot], st));
    level_slots_[phase] = std::max(level_slots_[phase], slot + 1);
}
// out[0] = the sweep tasks (0 for the factorisation), out[1 + l] = tree level l, milliseconds; returns the count
int Device::level_times(int phase, double *out, int cap) {
    HC(hipSetDevice(device));
    const int nl = (int)levels_.size();
    if (!env_.level_mark || phase < 0 || phase > 2 || level_slots_[phase] < (phase == 0 ? nl + 1 : nl + 2)) return 0;
    HC(hipDeviceSynchronize());
    auto &v = ev_level_[phase];
    auto dt = [&](int a, int b) { float ms = 0; HC(hipEventElapsedTime(&ms, v[a], v[b])); return (double)ms; };
    for (int k = 0; k <= nl && k < cap; k++) {
        if (phase == 0) out[k] = k == 0 ? 0.0 : dt(k - 1, k);                       // slots: start of level l = l, end = nl
        else if (phase == 1) out[k] = dt(k, k + 1);                                  // slot 0 = start, 1 + l = start of level l, 1 + nl = end
        else out[k] = k == 0 ? dt(nl, nl + 1) : dt(nl - k, nl - k + 1);              // processing order: level nl-1 .. 0, tasks
    }
    return std::min(nl + 1, cap);
}

void Device::solve_phase(const double *d_B, long long ldb, long long nrhs, double *d_Xout, long long ldx_out, int phase) {
    HC(hipSetDevice(device));
    if (!sharded()) throw std::invalid_argument("gmrfx_solve_phase needs a sharded handle (shard_world > 1, or shard_min_top > 0)");
    if (nrhs <= 0 || nrhs > 64) throw std::invalid_argument("sharded solves take 1..64 right-hand sides per call");
    const int nr = (int)nrhs, ldx = nr, nl = (int)levels_.size();
    const int split = std::min<int>(S_->shard_level, nl);
    const long long n = S_->n;
    HC(hipEventRecord(ev_[0], stream));
    if (phase == 0 || phase == 10) ensure_rhs_capacity(nrhs);
    const SweepLane ln = lane(0);
    if (phase == 0) {                                     // transpose in + forward over the own subtrees
        start_inverse_async();
        ensure_rdiag(stream);
        ensure_dtile(stream);
        launch_permute(stream, d_iperm_, (int)n, const_cast<double *>(d_B), ldb, ln.X, nr, ldx, 0);
        forward(ln, nr, ldx, 0, split, false);
    } else if (phase >= 100 && phase < 100 + (nl - split)) {       // forward, top level split + (phase - 100)
        const int lev = split + phase - 100;
        forward(ln, nr, ldx, lev, lev + 1, false);
    } else if (phase >= 200 && phase < 200 + (nl - split)) {       // backward, top level split + (phase - 200)
        const int lev = split + phase - 200;
        backward(ln, nr, ldx, true, lev + 1, lev);
    } else if (phase == 2) {                              // backward over the own subtrees
        backward(ln, nr, ldx, true, split, 0);
    } else if (phase == 10) {                             // F.UP \ z: z is taken in elimination order as is, no forward sweep
        start_inverse_async();
        ensure_rdiag(stream);
        ensure_dtile(stream);
        launch_permute(stream, nullptr, (int)n, const_cast<double *>(d_B), ldb, ln.X, nr, ldx, 0);
    } else if (phase >= 300 && phase < 300 + (nl - split)) {       // backward-only solve, top level split + (phase - 300)
        const int lev = split + phase - 300;
        backward(ln, nr, ldx, false, lev + 1, lev);
    } else if (phase == 12) {                             // backward-only solve over the own subtrees
        backward(ln, nr, ldx, false, split, 0);
    } else if (phase == 3) {                              // transpose out (rank 0, after the gather)
        launch_permute(stream, d_iperm_, (int)n, d_Xout, ldx_out, ln.X, nr, ldx, 1);
    } else throw std::invalid_argument("solve phase must be 0, 2, 3, 10, 12, 100 + k, 200 + k or 300 + k (k = top level)");
    HC(hipEventRecord(ev_[1], stream));
    if (!async_phases_) {
        HC(hipStreamSynchronize(stream));
        HC(hipGetLastError());
        float ms = 0;
        HC(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
        ms_solve = (phase == 0 || phase == 10) ? ms : ms_solve + ms;
    }
    last_nrhs = nrhs;
}

// One pass of at most 64 columns on lane ln: dB (column-major, original ordering) -> ln.X (elimination order, row-major), the
// sweeps, and back to dXo. mode 0: full solve, X = P b; 1: backward only (F.UP \ z), z is taken in elimination order as is.
void Device::sweep_pass(const SweepLane &ln, const Event *ev, const double *dB, long long ldin, double *dXo, long long ldout, int nr, int mode,
                        const MemberLayout *ml) {
    const int n = (int)S_->n, ldx = nr, nl = (int)levels_.size();
    auto mark = [&](int k) { if (ev) HC(hipEventRecord(ev[k], ln.st)); };
    mark(0);
    if (ml) launch_batch_permute(ln.st, mode == 0 ? d_iperm_ : nullptr, n, (int)ml->n_member, const_cast<double *>(dB), ldin, ml->sin, ln.X, nr, ldx, 0);
    else launch_permute(ln.st, mode == 0 ? d_iperm_ : nullptr, n, const_cast<double *>(dB), ldin, ln.X, nr, ldx, 0);
    mark(1);
    if (mode == 0) forward(ln, nr, ldx, 0, nl, false);
    mark(2);
    backward(ln, nr, ldx, mode == 0, nl, 0);
    mark(3);
    if (ml) launch_batch_permute(ln.st, d_iperm_, n, (int)ml->n_member, dXo, ldout, ml->sout, ln.X, nr, ldx, 1);
    else launch_permute(ln.st, d_iperm_, n, dXo, ldout, ln.X, nr, ldx, 1);
    mark(4);
}

void Device::solve(const double *B, long long ldb, long long nrhs, double *X, long long ldx_out, bool on_device, int mode,
                   const MemberLayout *ml) {
    HC(hipSetDevice(device));
    if (sharded()) throw std::invalid_argument("sharded handle: use gmrfx_solve_phase (phases with exchanges in between, gmrfx/shard.py)");
    if (ml && !on_device) throw std::invalid_argument("member-strided solves take device arrays");
    if (nrhs <= 0) return;
    const long long n = S_->n;
    ensure_rhs_capacity(nrhs);
    start_inverse_async();
    ensure_rdiag(stream);      // (on the main stream, before the lanes fork)
    ensure_dtile(stream);
    const double *dB = B;
    double *dXo = X;
    long long ldin = ldb, ldout = ldx_out;
    if (!on_device) {
        const long long need = n * nrhs;
        ensure_io(need);
        if (ldb == n) HC(hipMemcpyAsync(d_io_, B, (size_t)need * sizeof(double), hipMemcpyHostToDevice, stream));
        else HC(hipMemcpy2DAsync(d_io_, n * sizeof(double), B, ldb * sizeof(double), n * sizeof(double), nrhs, hipMemcpyHostToDevice, stream));
        dB = d_io_; dXo = d_io_; ldin = n; ldout = n;
    }
    double t_perm = 0, t_fwd = 0, t_bwd = 0;
    // passes of pass_width() = 64 columns, alternating between the two lanes when there is more than one pass
    const int PW = pass_width(nrhs);
    const bool two = nrhs > PW && d_Xb_ != nullptr;
    const SweepLane lanes[2] = {lane(0), lane(1)};
    if (two) {
        // lane 1 starts after everything already enqueued on the main stream (factorisation, upload of B)
        HC(hipEventRecord(ev_ready_, stream));
        HC(hipStreamWaitEvent(stream3, ev_ready_, 0));
    }
    bool busy[2] = {false, false};
    auto collect = [&](int ln) {
        if (!busy[ln]) return;
        HC(hipEventSynchronize(ev_lane_[ln][4]));
        float a, b, c, d;
        HC(hipEventElapsedTime(&a, ev_lane_[ln][0], ev_lane_[ln][1]));
        HC(hipEventElapsedTime(&b, ev_lane_[ln][1], ev_lane_[ln][2]));
        HC(hipEventElapsedTime(&c, ev_lane_[ln][2], ev_lane_[ln][3]));
        HC(hipEventElapsedTime(&d, ev_lane_[ln][3], ev_lane_[ln][4]));
        t_perm += a + d; t_fwd += b; t_bwd += c;
        busy[ln] = false;
    };
    HC(hipEventRecord(ev_[0], stream));
    int pass = 0;
    for (long long j0 = 0; j0 < nrhs; j0 += PW, pass++) {
        const int ln = two ? (pass & 1) : 0;
        collect(ln);                         // the lane's previous pass has finished: its buffers are free
        sweep_pass(lanes[ln], ev_lane_[ln], dB + j0 * ldin, ldin, dXo + j0 * ldout, ldout, (int)std::min<long long>(PW, nrhs - j0), mode, ml);
        busy[ln] = true;
    }
    if (two) {
        HC(hipEventRecord(ev_done1_, stream3));
        HC(hipStreamWaitEvent(stream, ev_done1_, 0));
    }
    HC(hipEventRecord(ev_[1], stream));
    collect(0);
    collect(1);
    HC(hipStreamSynchronize(stream));
    float wall = 0;
    HC(hipEventElapsedTime(&wall, ev_[0], ev_[1]));
    HC(hipGetLastError());
    if (!on_device) {
        const long long need = n * nrhs;
        if (ldx_out == n) HC(hipMemcpyAsync(X, d_io_, (size_t)need * sizeof(double), hipMemcpyDeviceToHost, stream));
        else HC(hipMemcpy2DAsync(X, ldx_out * sizeof(double), d_io_, n * sizeof(double), n * sizeof(double), nrhs, hipMemcpyDeviceToHost, stream));
        HC(hipStreamSynchronize(stream));
    }
    // per-phase times are sums over the passes; with two lanes the passes overlap, so the totals are the
    // elapsed time on the device from the first launch to the last completion
    ms_perm = t_perm; ms_fwd = t_fwd; ms_bwd = t_bwd;
    if (mode == 0) ms_solve = two ? wall : t_perm + t_fwd + t_bwd; else ms_bsolve = two ? wall : t_perm + t_bwd;
    last_nrhs = nrhs;
}

// log det Q = 2 sum log L_jj: two small kernels over the factor's diagonal + one scalar copied to pinned host memory. The result
// is kept per factorisation; the pipelined factor + solve call enqueues it on the side stream beside the backward sweep.
void Device::enqueue_logdet(hipStream_t st, bool timed) {
    if (!h_logdet_) {
        h_logdet_.alloc(1);
        ev_logdet_.create(hipEventDisableTiming);
    }
    const int nparts = (int)std::min<long long>(1024, std::max<long long>(1, (S_->n + 255) / 256));
    if (timed) HC(hipEventRecord(ev_[0], st));
    launch_logdet(st, d_L_, ds_.diagoff, d_owncol_, (int)S_->n, d_part_, nparts, d_part_ + 1024);
    if (timed) HC(hipEventRecord(ev_[1], st));
    HC(hipMemcpyAsync(h_logdet_, d_part_ + 1024, sizeof(double), hipMemcpyDeviceToHost, st));
    HC(hipEventRecord(ev_logdet_, st));
    logdet_for_ = factor_serial_;
}
double Device::logdet() {
    HC(hipSetDevice(device));
    if (logdet_for_ != factor_serial_ || !h_logdet_) {
        enqueue_logdet(stream, true);
        HC(hipEventSynchronize(ev_logdet_));
        float ms; HC(hipEventElapsedTime(&ms, ev_[0], ev_[1])); ms_logdet = ms;
    } else HC(hipEventSynchronize(ev_logdet_));
    return *h_logdet_;
}

// pattern of Q and the partial-sum buffers of the quadratic-form kernels (grown geometrically)
void Device::prepare_quadform(long long nvec) {
    const Symbolic &S = *S_;
    if (!d_in_colptr_) {
        d_in_colptr_ = dalloc<long long>(S.in_colptr.size());
        d_in_row_ = dalloc<int>(std::max<size_t>(S.in_row.size(), 1));
        HC(hipMemcpyAsync(d_in_colptr_, S.in_colptr.data(), S.in_colptr.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
        HC(hipMemcpyAsync(d_in_row_, S.in_row.data(), S.in_row.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        HC(hipStreamSynchronize(stream));      // (the host vectors may move; first call only)
    }
    const int nblk = quadform_blocks((int)S.n);
    if (nvec > qf_cap_) {
        const long long cap = std::max<long long>(nvec, 2 * qf_cap_);     // geometric growth, the old buffers are freed
        qf_cap_ = 0;        // (a failed second allocation must not leave the pair with different sizes behind one capacity)
        regrow(d_qf_part_, (size_t)cap * nblk, &bytes_total);
        regrow(d_qf_out_, (size_t)cap, &bytes_total);
        qf_cap_ = cap;
    }
}

// One evaluation of the hyper-parameter loop as ONE call (gmrfx_refactorize_logpdf_dev): new values -> numeric factorisation,
// r' Q r for nvec vectors and log det Q -- logpdf(::WorkspaceGMRF, z) = -r'Qr / 2 + logdet(Q) / 2 - n log(2 pi) / 2,
// src/workspace/workspace_gmrf.jl:288-292, with ensure_numeric! inside (gmrf_workspace.jl:170-178). The quadratic forms only
// need Q's values: they run on the side stream beside the factorisation; the log-determinant follows the factorisation on the
// main stream; ONE synchronisation, the scalars arrive in pinned memory. Same kernels: same bits as the three calls.
void Device::refactorize_logpdf(const double *d_nz, const double *d_X, long long ldx, long long nvec, const double *d_mu, double *quad_out,
                                double *logdet_out) {
    HC(hipSetDevice(device));
    const Symbolic &S = *S_;
    if (sharded()) throw std::invalid_argument("sharded handle: use the phase entry points (gmrfx/shard.py)");
    if (nvec < 0 || nvec > 65535) throw std::invalid_argument("refactorize_logpdf: 0..65535 vectors per call");
    if (nvec > 0 && ldx < S.n) throw std::invalid_argument("refactorize_logpdf: ldx < n");
    if (stream != own_stream_) throw std::invalid_argument("refactorize_logpdf: not on a caller's stream");
    if (nvec > 0) {
        prepare_quadform(nvec);
        h_qf_.grow(nvec, 16);
        HC(hipEventRecord(ev_ready_, stream));
        HC(hipStreamWaitEvent(stream2, ev_ready_, 0));
        launch_quadform(stream2, (int)S.n, d_in_colptr_, d_in_row_, d_nz, S.in_use, d_X, ldx, (int)nvec, d_mu, d_qf_part_, d_qf_out_);
        HC(hipMemcpyAsync(h_qf_, d_qf_out_, (size_t)nvec * sizeof(double), hipMemcpyDeviceToHost, stream2));
        ev_qf_.ensure(hipEventDisableTiming);
        HC(hipEventRecord(ev_qf_, stream2));
    }
    begin_factor(d_nz);
    factor_levels(0, (int)levels_.size(), false);
    enqueue_factor_tail();
    inverse_pending = true;
    enqueue_logdet(stream, false);
    if (nvec > 0) HC(hipStreamWaitEvent(stream, ev_qf_, 0));
    HC(hipStreamSynchronize(stream));
    finish_factor();
    for (long long k = 0; k < nvec; k++) quad_out[k] = h_qf_[k];
    if (logdet_out) *logdet_out = *h_logdet_;
}

void Device::quadform(const double *d_nz, const double *d_X, long long ldx, long long nvec, const double *d_mu, double *out_host) {
    HC(hipSetDevice(device));
    const Symbolic &S = *S_;
    if (nvec <= 0) return;
    if (nvec > 65535) throw std::invalid_argument("quadform: at most 65535 vectors per call");
    if (ldx < S.n) throw std::invalid_argument("quadform: ldx < n");
    if (!d_nz) {
        if (!nz_held_) throw std::invalid_argument("quadform: the handle does not hold Q's values (last refactorisation read a caller device buffer): pass them");
        d_nz = d_nz_;
    }
    prepare_quadform(nvec);
    HC(hipEventRecord(ev_[0], stream));
    launch_quadform(stream, (int)S.n, d_in_colptr_, d_in_row_, d_nz, S.in_use, d_X, ldx, (int)nvec, d_mu, d_qf_part_, d_qf_out_);
    HC(hipEventRecord(ev_[1], stream));
    HC(hipMemcpyAsync(out_host, d_qf_out_, (size_t)nvec * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
    float ms; HC(hipEventElapsedTime(&ms, ev_[0], ev_[1])); ms_quadform = ms;
}

void Device::selinv_begin() {
    const Symbolic &S = *S_;
    start_inverse_async();
    wait_inverse(stream);
    if (!inverse_full_) {      // the sweeps only need inv_cap_-column inverses; the Takahashi step needs all of L11^-1
        invert_diag_blocks(stream, inv_cap_, 1 << 30);
        inverse_full_ = true;
    }
    if (!d_Z_) d_Z_ = dalloc<double>((size_t)l_size_);
    // workspaces: small fronts: Yh = r x 64 per front; big fronts: Yt and Z21t = (r-c) x c each
    if (!d_yoff_) {
        std::vector<long long> yoff(S.nsuper, 0);
        long long mx = 0;
        for (i32 l = 0; l < S.nlevels; l++) {
            long long off = 0;
            const i64 lf = S.sel_levelptr[l], cnt = S.sel_levelptr[l + 1] - lf;
            for (i64 k = 0; k < cnt; k++) {
                i32 s = S.sel_levellist[lf + k];
                yoff[s] = off;
                off += k < S.sel_level_nsmall[l] ? (long long)S.nrows(s) * NB : 2LL * (S.nrows(s) - S.ncols(s)) * S.ncols(s);
            }
            mx = std::max(mx, off);
        }
        if (mx > tmp_cap_) { regrow(d_tmp_, (size_t)mx, &bytes_total); tmp_cap_ = mx; }
        d_yoff_ = dalloc<long long>(std::max<size_t>(yoff.size(), 1));
        HC(hipMemcpyAsync(d_yoff_, yoff.data(), yoff.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
        HC(hipStreamSynchronize(stream));
    }
    HC(hipMemsetAsync(d_Z_, 0, (size_t)l_size_ * sizeof(double) + kPairSlackBytes, stream));
}

void Device::selinv_levels(int hi, int lo) {
    const Symbolic &S = *S_;
    DevSym dsz = ds_;            // the selected inversion has its own slot layout in the contribution-block arena
    dsz.cbptr = d_zbptr_;
    for (int l = hi - 1; l >= lo; l--) {
        // all fronts of the level (subtree members included): small first, then big
        const int sfirst = (int)S.sel_levelptr[l], scount = (int)(S.sel_levelptr[l + 1] - S.sel_levelptr[l]);
        const int snsmall = S.sel_level_nsmall[l];
        const int *list = d_sel_levellist_ + sfirst + snsmall;
        const int nf = scount - snsmall;
        // big fronts: whole-front step through the dense inverse (selinv.hip, k_sel_dense).
        // Yt lives at d_tmp_ + yoff[s], Z21t right behind it (offset (r-c)*c): pass both bases.
        // (geometry over the level's fronts of the SELECTED-INVERSION list: the factor's level list of a sharded handle
        //  leaves out the distributed root, which the owner still inverts)
        if (env_.level_mark) launch_level_mark(stream, 4, l);      // (profiling aid: tools/cfg3_profile.py cuts the trace into levels)
        launch_sel_gather(stream, d_selrec_, dsz, list, nf, sel_max_trail_[l], d_Z_, d_cb_);
        for (int phase = 0; phase < 3; phase++)
            launch_sel_dense(stream, dsz, list, nf, phase, sel_max_cols_[l], sel_max_trail_[l], d_L_, d_Z_, d_cb_, d_tmp_,
                             d_tmp_, d_yoff_);
        // small fronts of the level (<= 128 rows, <= 64 columns: one block step)
        if (snsmall > 0) {
            const int *sl = d_sel_levellist_ + sfirst;
            launch_sel_gather(stream, d_selrec_, dsz, sl, snsmall, 128, d_Z_, d_cb_);
            launch_trsm(stream, dsz, d_sel_frec_ + sfirst, snsmall, 0, 1, 128, d_L_, d_tmp_, d_yoff_, FrontArg{0, 0, 0, 0, 0, 0, 0});
            launch_sel_symm(stream, dsz, sl, snsmall, 0, 128, d_Z_, d_cb_, d_tmp_, d_yoff_);
            launch_sel_diag(stream, dsz, sl, snsmall, 0, d_L_, d_Z_, d_tmp_, d_yoff_);
        }
    }
}

void Device::selinv_compute() {
    HC(hipSetDevice(device));
    if (selinv_valid) return;
    if (sharded()) throw std::invalid_argument("sharded handle: the selected inversion runs in phases with exchanges in between (gmrfx_selinv_phase, gmrfx/shard.py)");
    selinv_begin();
    HC(hipEventRecord(ev_[0], stream));
    selinv_levels((int)levels_.size(), 0);
    HC(hipEventRecord(ev_[1], stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms; HC(hipEventElapsedTime(&ms, ev_[0], ev_[1])); ms_selinv = ms;
    selinv_valid = true;
}

void Device::selinv_phase(int what, int hi, int lo) {
    HC(hipSetDevice(device));
    if (!sharded()) throw std::invalid_argument("gmrfx_selinv_phase needs a sharded handle (shard_world > 1, or shard_min_top > 0)");
    const int nl = (int)levels_.size();
    if (what != 0 && !selinv_begun_)       // (phases 1-3 launch kernels on the workspaces phase 0 allocates)
        throw std::invalid_argument("selinv phase 1, 2 or 3 before phase 0 (begin) since the last refactorisation");
    if (what == 0) {
        if (!factorized) throw std::invalid_argument("selinv phase 0 before the factorisation has finished");
        selinv_valid = false;
        selinv_begin();
        selinv_begun_ = true;
        ms_selinv = 0;
    } else if (what == 1) {
        if (hi < 0 || hi >= nl) throw std::invalid_argument("selinv phase: level out of range");
        DevSym dsz = ds_;
        dsz.cbptr = d_zbptr_;
        const int a = fc_levelptr_[hi], b = fc_levelptr_[hi + 1];
        launch_sel_gather(stream, d_selrec_, dsz, d_fchild_ + a, b - a, fc_maxtrail_[hi], d_Z_, d_cb_);
    } else if (what == 2) {
        if (lo < 0 || hi > nl || lo > hi) throw std::invalid_argument("selinv phase: level range out of bounds");
        HC(hipEventRecord(ev_[0], stream));
        selinv_levels(hi, lo);
        HC(hipEventRecord(ev_[1], stream));
        if (!async_phases_) {
            HC(hipStreamSynchronize(stream));
            float ms; HC(hipEventElapsedTime(&ms, ev_[0], ev_[1])); ms_selinv += ms;
        }
    } else if (what == 3) {
        selinv_valid = true;
    } else throw std::invalid_argument("selinv phase must be 0 (begin), 1 (gather for other ranks), 2 (own levels) or 3 (end)");
    if (!async_phases_) HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
}

void Device::selinv_diag(double *out_host) {
    HC(hipSetDevice(device));
    const long long n = S_->n;
    if (n > io_cap_) { regrow(d_io_, (size_t)n, &bytes_total); io_cap_ = n; }
    launch_gather_diag(stream, d_Z_, ds_.diagoff, ds_.perm, (int)n, d_io_);
    HC(hipMemcpyAsync(out_host, d_io_, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
}

void Device::gather_z(const long long *offsets_host, long long cnt, double *out_host) {
    HC(hipSetDevice(device));
    if (cnt <= 0) return;
    DevBuf<long long> d_off;
    DevBuf<double> d_out;
    d_off.alloc((size_t)cnt);
    d_out.alloc((size_t)cnt);
    HC(hipMemcpyAsync(d_off, offsets_host, (size_t)cnt * sizeof(long long), hipMemcpyHostToDevice, stream));
    launch_gather(stream, d_Z_, d_off, cnt, d_out);
    HC(hipMemcpyAsync(out_host, d_out, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
}

void Device::weighted_z_sums(const long long *segptr_host, long long nseg, const long long *off_host, const double *w_host,
                             double *out_host) {
    HC(hipSetDevice(device));
    if (nseg <= 0) return;
    if (nseg > 0x7fffffffLL) throw std::invalid_argument("too many segments");
    const long long cnt = segptr_host[nseg];
    DevBuf<long long> bseg, boff;
    DevBuf<double> bw, bout;
    bseg.alloc((size_t)nseg + 1);
    boff.alloc((size_t)cnt);
    bw.alloc((size_t)cnt);
    bout.alloc((size_t)nseg);
    HC(hipMemcpyAsync(bseg, segptr_host, (size_t)(nseg + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
    HC(hipMemcpyAsync(boff, off_host, (size_t)cnt * sizeof(long long), hipMemcpyHostToDevice, stream));
    HC(hipMemcpyAsync(bw, w_host, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, stream));
    launch_seg_wsum(stream, d_Z_, bseg, nseg, boff, bw, bout);
    HC(hipMemcpyAsync(out_host, bout, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
}

long long Device::rowdiag_plan_create(const long long *segptr_host, long long nseg, const long long *off_host, const int *p_host,
                                      const int *q_host, long long nvals) {
    HC(hipSetDevice(device));
    if (nseg > 0x7fffffffLL) throw std::invalid_argument("too many rows");
    RowDiagPlan P;
    P.nseg = nseg; P.cnt = nseg > 0 ? segptr_host[nseg] : 0; P.nvals = nvals;
    P.seg.alloc((size_t)nseg + 1);
    P.off.alloc((size_t)P.cnt);
    P.p.alloc((size_t)P.cnt);
    P.q.alloc((size_t)P.cnt);
    P.vals.alloc((size_t)nvals);
    P.out.alloc((size_t)nseg);
    HC(hipMemcpyAsync(P.seg, segptr_host, (size_t)(nseg + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
    HC(hipMemcpyAsync(P.off, off_host, (size_t)P.cnt * sizeof(long long), hipMemcpyHostToDevice, stream));
    HC(hipMemcpyAsync(P.p, p_host, (size_t)P.cnt * sizeof(int), hipMemcpyHostToDevice, stream));
    HC(hipMemcpyAsync(P.q, q_host, (size_t)P.cnt * sizeof(int), hipMemcpyHostToDevice, stream));
    HC(hipStreamSynchronize(stream));
    for (size_t k = 0; k < rd_plans_.size(); k++)
        if (!rd_plans_[k].seg) { rd_plans_[k] = std::move(P); return (long long)k; }
    rd_plans_.push_back(std::move(P));
    return (long long)rd_plans_.size() - 1;
}

void Device::rowdiag_plan_apply(long long id, const double *values_host, double *out_host) {
    HC(hipSetDevice(device));
    if (id < 0 || id >= (long long)rd_plans_.size() || !rd_plans_[id].seg) throw std::invalid_argument("unknown row-diag plan");
    const RowDiagPlan &P = rd_plans_[id];
    if (P.nseg <= 0) return;
    HC(hipMemcpyAsync(P.vals, values_host, (size_t)P.nvals * sizeof(double), hipMemcpyHostToDevice, stream));
    launch_seg_wsum_pairs(stream, d_Z_, P.seg, P.nseg, P.off, P.p, P.q, P.vals, P.out);
    HC(hipMemcpyAsync(out_host, P.out, (size_t)P.nseg * sizeof(double), hipMemcpyDeviceToHost, stream));
    HC(hipStreamSynchronize(stream));
}

void Device::rowdiag_plan_free(long long id) {
    if (id < 0 || id >= (long long)rd_plans_.size() || !rd_plans_[id].seg) return;
    rd_plans_[id] = RowDiagPlan{};
}

void Device::dense_apply(const double *d_D, const double *d_T, double *d_R, long long n1, long long n2) {
    HC(hipSetDevice(device));
    launch_dense_apply(stream, d_D, d_T, d_R, (int)n1, n2);
    HC(hipGetLastError());
    HC(hipStreamSynchronize(stream));
}
void Device::transpose(const double *d_src, double *d_dst, long long rows, long long cols) {
    HC(hipSetDevice(device));
    launch_transpose(stream, d_src, d_dst, rows, cols);
    HC(hipGetLastError());
    HC(hipStreamSynchronize(stream));
}

void Device::copy_factor(double *out_host) {
    HC(hipSetDevice(device));
    HC(hipMemcpy(out_host, d_L_, (size_t)l_size_ * sizeof(double), hipMemcpyDeviceToHost));
}

// ---- batched handles (gmrfx_create_batched): the handle's structure is the forest of diag(Q_1 .. Q_B); these are the only places
// that see the members one by one (batch.hip) --------------------------------------------------------------------------------------
void Device::set_batch(int nbatch, long long n_member, long long nnz_member) {
    HC(hipSetDevice(device));
    const Symbolic &S = *S_;
    if (nbatch < 1 || n_member * nbatch != S.n || nnz_member * nbatch != S.nnz_in) throw std::invalid_argument("set_batch: sizes do not match the forest");
    nbatch_ = nbatch; nmember_ = n_member; nnz_member_ = nnz_member;
    d_bpsum_ = dalloc<double>((size_t)nbatch * batch_diag_parts((int)n_member));
    d_bpbad_ = dalloc<int>((size_t)nbatch * batch_diag_parts((int)n_member));
    d_bdiag_ = dalloc<double>(2 * (size_t)nbatch);
    h_bdiag_.alloc(2 * (long long)nbatch);
    ev_bdiag_.create(hipEventDisableTiming);
    // the member's pattern = the forest's first n_member columns (rows unshifted)
    d_bin_colptr_ = dalloc<long long>((size_t)n_member + 1);
    d_bin_row_ = dalloc<int>((size_t)std::max<long long>(nnz_member, 1));
    HC(hipMemcpyAsync(d_bin_colptr_, S.in_colptr.data(), ((size_t)n_member + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
    if (nnz_member > 0) HC(hipMemcpyAsync(d_bin_row_, S.in_row.data(), (size_t)nnz_member * sizeof(int), hipMemcpyHostToDevice, stream));
    HC(hipStreamSynchronize(stream));
}

void Device::enqueue_batch_diag(hipStream_t st) {
    double *ld = d_bdiag_;
    long long *info = reinterpret_cast<long long *>(d_bdiag_ + nbatch_);
    launch_batch_diag(st, d_L_, ds_.diagoff, (int)nmember_, nbatch_, d_bpsum_, d_bpbad_, ld, info);
    HC(hipMemcpyAsync(h_bdiag_, d_bdiag_, 2 * (size_t)nbatch_ * sizeof(double), hipMemcpyDeviceToHost, st));
    HC(hipEventRecord(ev_bdiag_, st));
    bdiag_for_ = factor_serial_;
}

void Device::batch_diag(double *logdet_out, long long *info_out) {
    HC(hipSetDevice(device));
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    if (bdiag_for_ != factor_serial_) enqueue_batch_diag(stream);
    HC(hipEventSynchronize(ev_bdiag_));
    HC(hipGetLastError());
    read_batch_diag(logdet_out, info_out);
}
// h_bdiag_ (valid once ev_bdiag_ has passed): nbatch log dets, then nbatch info words; either output may be null
void Device::read_batch_diag(double *logdet_out, long long *info_out) const {
    const long long *hi = reinterpret_cast<const long long *>(h_bdiag_ + nbatch_);
    for (int k = 0; k < nbatch_; k++) {
        if (logdet_out) logdet_out[k] = h_bdiag_[k];
        if (info_out) info_out[k] = hi[k];
    }
}

void Device::prepare_batch_quadform(long long npairs) {
    const long long nblk = batch_quadform_blocks((int)nmember_);
    if (npairs > bqf_cap_) {
        const long long cap = std::max<long long>(npairs, 2 * bqf_cap_);
        bqf_cap_ = 0;
        regrow(d_bqf_part_, (size_t)(cap * nblk), &bytes_total);
        regrow(d_bqf_out_, (size_t)cap, &bytes_total);
        bqf_cap_ = cap;
    }
    h_bqf_.grow(npairs, 64);
}

void Device::enqueue_batch_quadform(hipStream_t st, const double *d_nz, const double *d_X, long long ldx, long long sx, long long nvec,
                                    const double *d_mu) {
    launch_batch_quadform(st, (int)nmember_, d_bin_colptr_, d_bin_row_, d_nz, nnz_member_, S_->in_use, d_X, ldx, sx, (int)nvec, nbatch_, d_mu,
                          d_bqf_part_, d_bqf_out_);
    HC(hipMemcpyAsync(h_bqf_, d_bqf_out_, (size_t)(nvec * nbatch_) * sizeof(double), hipMemcpyDeviceToHost, st));
}

void Device::batch_quadform(const double *d_nz, const double *d_X, long long ldx, long long sx, long long nvec, const double *d_mu,
                            double *quad_out) {
    HC(hipSetDevice(device));
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    if (nvec <= 0) return;
    if (!d_nz) {
        if (!nz_held_) throw std::invalid_argument("batch_quadform: the handle does not hold Q's values (last refactorisation read a caller device buffer): pass them");
        d_nz = d_nz_;
    }
    prepare_batch_quadform(nvec * nbatch_);
    HC(hipEventRecord(ev_[0], stream));
    enqueue_batch_quadform(stream, d_nz, d_X, ldx, sx, nvec, d_mu);
    HC(hipEventRecord(ev_[1], stream));
    HC(hipStreamSynchronize(stream));
    HC(hipGetLastError());
    float ms; HC(hipEventElapsedTime(&ms, ev_[0], ev_[1])); ms_quadform = ms;
    for (long long k = 0; k < nvec * nbatch_; k++) quad_out[k] = h_bqf_[k];
}

// One batched evaluation of the hyper-parameter loop (gmrfx_batch_refactorize_logpdf_dev), the batched twin of refactorize_logpdf:
// the forest is refactored on the main stream, the members' quadratic forms run beside it on the side stream, the per-member log
// det / pivot status follows the factorisation; ONE synchronisation. The same launches as batch_refactorize + batch_quadform +
// batch_logdet: the same bits.
void Device::batch_refactorize_logpdf(const double *d_nz, const double *d_X, long long ldx, long long sx, long long nvec, const double *d_mu,
                                      double *quad_out, double *logdet_out, long long *info_out) {
    HC(hipSetDevice(device));
    if (!h_bdiag_) throw std::invalid_argument("not a batched handle");
    if (stream != own_stream_) throw std::invalid_argument("batch_refactorize_logpdf: not on a caller's stream");
    if (nvec > 0) {
        prepare_batch_quadform(nvec * nbatch_);
        HC(hipEventRecord(ev_ready_, stream));
        HC(hipStreamWaitEvent(stream2, ev_ready_, 0));
        enqueue_batch_quadform(stream2, d_nz, d_X, ldx, sx, nvec, d_mu);
        ev_qf_.ensure(hipEventDisableTiming);
        HC(hipEventRecord(ev_qf_, stream2));
    }
    begin_factor(d_nz);
    factor_levels(0, (int)levels_.size(), false);
    enqueue_factor_tail();
    inverse_pending = true;
    enqueue_batch_diag(stream);
    if (nvec > 0) HC(hipStreamWaitEvent(stream, ev_qf_, 0));
    HC(hipStreamSynchronize(stream));
    finish_factor();
    for (long long k = 0; k < nvec * nbatch_; k++) quad_out[k] = h_bqf_[k];
    read_batch_diag(logdet_out, info_out);
}

}  // namespace gmrfx
