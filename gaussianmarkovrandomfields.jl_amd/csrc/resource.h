// resource.h -- move-only owners of what a handle takes from the HIP runtime: a device buffer, a page-locked host buffer, an
// event, a stream. Each holds one resource or none and releases it on destruction, ignoring errors. Move assignment swaps: what
// the target held before goes when the source does.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace gmrfx {

void hip_check(hipError_t e, const char *what);

// One hipMalloc block of max(count * sizeof(T), min_bytes) + 16 bytes: kernels that load rows in pairs (16 bytes per lane) may
// read one element past the last one; the value is never used, but the address must be mapped. With a ledger the bytes are
// added to it on allocation and taken off it on release.
template <class T> class DevBuf {
public:
    DevBuf() = default;
    ~DevBuf() { reset(); }
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_), ledger_(o.ledger_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); std::swap(ledger_, o.ledger_); return *this; }
    // (both release what the buffer held before; a failure leaves it empty)
    void alloc(size_t count, double *ledger = nullptr, size_t min_bytes = sizeof(T)) {
        hip_check(malloc_block(count, ledger, min_bytes), "hipMalloc(&p, bytes)");
    }
    // false (and no sticky HIP error) when the block does not fit: for callers to whom that is an answer
    bool try_alloc(size_t count, double *ledger = nullptr, size_t min_bytes = sizeof(T)) {
        if (malloc_block(count, ledger, min_bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    void reset() {
        if (!p_) return;
        if (ledger_) *ledger_ -= (double)bytes_;
        (void)hipFree(p_);
        p_ = nullptr;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    hipError_t malloc_block(size_t count, double *ledger, size_t min_bytes) {
        reset();
        void *p = nullptr;
        const size_t bytes = std::max(count * sizeof(T), min_bytes) + 16;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        p_ = (T *)p; bytes_ = bytes; ledger_ = ledger;
        if (ledger_) *ledger_ += (double)bytes_;
        return e;
    }
    T *p_ = nullptr;
    size_t bytes_ = 0;
    double *ledger_ = nullptr;
};

constexpr size_t kTableMinBytes = 8;      // the size rule of a handle's tables: 8 bytes at least (+ the 16 of slack)
// dst = a device copy of count entries of src, on the ledger's books (an element type of the same size is copied as bytes:
// std::int64_t and long long, std::uint8_t and unsigned char)
template <class T, class U> void dev_upload(DevBuf<T> &dst, const U *src, size_t count, double *ledger) {
    static_assert(sizeof(T) == sizeof(U), "dev_upload copies bytes");
    dst.alloc(count, ledger, kTableMinBytes);
    if (count > 0) hip_check(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
}
template <class T, class U> void dev_upload(DevBuf<T> &dst, const std::vector<U> &src, double *ledger) { dev_upload(dst, src.data(), src.size(), ledger); }

// Page-locked host memory of cap() elements.
template <class T> class PinnedBuf {
public:
    PinnedBuf() = default;
    ~PinnedBuf() { reset(); }
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    void alloc(long long count) {
        reset();
        hip_check(hipHostMalloc((void **)&p_, (size_t)std::max<long long>(count, 1) * sizeof(T), hipHostMallocDefault), "hipHostMalloc");
        cap_ = count;
    }
    // at least `count` elements (a fresh block holds `floor` at least; contents are not kept); a failed allocation leaves none
    void grow(long long count, long long floor) { if (count > cap_) alloc(std::max(count, floor)); }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr; cap_ = 0;
    }
    long long cap() const { return cap_; }
    operator T *() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T *p_ = nullptr;
    long long cap_ = 0;
};

class Event {
public:
    Event() = default;
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e_, o.e_); return *this; }
    void create(unsigned flags = hipEventDefault) {
        Event fresh;
        hip_check(hipEventCreateWithFlags(&fresh.e_, flags), "hipEventCreateWithFlags");
        *this = std::move(fresh);
    }
    void ensure(unsigned flags = hipEventDefault) { if (!e_) create(flags); }       // created on first use
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
    Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream &operator=(Stream &&o) noexcept { std::swap(s_, o.s_); return *this; }
    void create(unsigned flags) {
        Stream fresh;
        hip_check(hipStreamCreateWithFlags(&fresh.s_, flags), "hipStreamCreateWithFlags");
        *this = std::move(fresh);
    }
    void create(unsigned flags, int priority) {
        Stream fresh;
        hip_check(hipStreamCreateWithPriority(&fresh.s_, flags, priority), "hipStreamCreateWithPriority");
        *this = std::move(fresh);
    }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace gmrfx
