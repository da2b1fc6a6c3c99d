// Owners of device memory, events and streams (host only).  A device resource of the library lives in one of these three types and
// nowhere else: it is returned when its owner is released, moved into, reset to a default-constructed value or destroyed, so no
// list of fields to free exists anywhere.  The structs that kernels take by value (Workspace, GtTab, Msm16, ...) stay plain views
// filled from the owners beside them.
//
// THE RULE for scoped owners: an owner must not be released, or leave its scope, while a kernel in flight may still touch what it
// owns.  Synchronise the stream that uses it first; where that synchronisation sits on a path that can return early, synchronise
// or release() explicitly before the return.  (Error returns taken BEFORE the synchronisation lean on hipFree itself, which waits
// for the device; nothing else may.)
//
// The resource calls come in through ZKV_DEVMEM_API, a struct of static functions.  Unset, it is the HIP runtime, which also keeps
// the process-wide count of live allocations and bytes; a host test defines a counting fake before including this header.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/zkv.h"

#ifndef ZKV_DEVMEM_API
#include <hip/hip_runtime.h>
#include <atomic>
namespace zkv {
inline std::atomic<uint64_t> g_dev_live_allocs{0}, g_dev_live_bytes{0};
struct HipDevApi {
    typedef hipEvent_t event_t;
    typedef hipStream_t stream_t;
    static bool alloc(void** p, size_t bytes) {
        if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
        g_dev_live_allocs.fetch_add(1, std::memory_order_relaxed); g_dev_live_bytes.fetch_add(bytes, std::memory_order_relaxed);
        return true;
    }
    static void free(void* p, size_t bytes) {
        (void)hipFree(p);
        g_dev_live_allocs.fetch_sub(1, std::memory_order_relaxed); g_dev_live_bytes.fetch_sub(bytes, std::memory_order_relaxed);
    }
    static bool event_create(event_t* e, unsigned flags) { if (hipEventCreateWithFlags(e, flags) == hipSuccess) return true; (void)hipGetLastError(); *e = nullptr; return false; }
    static void event_destroy(event_t e) { (void)hipEventDestroy(e); }
    static bool stream_create(stream_t* s) { if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess) return true; (void)hipGetLastError(); *s = nullptr; return false; }
    static void stream_destroy(stream_t s) { (void)hipStreamDestroy(s); }
};
}  // namespace zkv
#define ZKV_DEVMEM_API zkv::HipDevApi
#endif

namespace zkv {

// A device buffer of T (bytes by default): grow(need) for staging, alloc(bytes) for tables and workspace rows of an exact size.
// Converts to T* where a pointer is wanted; as<U>() reads a byte buffer as another type.  Sizes are in bytes.
template <class T = uint8_t> class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() { if (p_) ZKV_DEVMEM_API::free(p_, cap_); p_ = nullptr; cap_ = 0; }
    // exactly `bytes` (0: stays empty), whatever was held before released first; ZKV_ERR_OOM (pending runtime error cleared) leaves the
    // buffer empty
    int alloc(size_t bytes) {
        release();
        void* q = nullptr;
        if (!bytes) return ZKV_OK;
        if (!ZKV_DEVMEM_API::alloc(&q, bytes)) return ZKV_ERR_OOM;
        p_ = (T*)q; cap_ = bytes;
        return ZKV_OK;
    }
    // at least `need`: nothing when it fits, else the old block goes BEFORE the new one is asked for (the peak does not rise) and the
    // new one has a quarter and 4 KB to spare
    int grow(size_t need) { return need <= cap_ ? ZKV_OK : alloc(need + need / 4 + 4096); }
    size_t cap() const { return cap_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    template <class U> U* as() const { return reinterpret_cast<U*>(p_); }
};

// An event; create(flags) returns ZKV_OK or ZKV_ERR_HIP (pending runtime error cleared).
class DevEvent {
    ZKV_DEVMEM_API::event_t e_ = nullptr;
public:
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { release(); e_ = o.e_; o.e_ = nullptr; } return *this; }
    ~DevEvent() { release(); }
    void release() { if (e_) ZKV_DEVMEM_API::event_destroy(e_); e_ = nullptr; }
    int create(unsigned flags = 0) { release(); return ZKV_DEVMEM_API::event_create(&e_, flags) ? ZKV_OK : ZKV_ERR_HIP; }
    operator ZKV_DEVMEM_API::event_t() const { return e_; }
};

// A non-blocking stream, in the same style.
class DevStream {
    ZKV_DEVMEM_API::stream_t s_ = nullptr;
public:
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    DevStream(DevStream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    DevStream& operator=(DevStream&& o) noexcept { if (this != &o) { release(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~DevStream() { release(); }
    void release() { if (s_) ZKV_DEVMEM_API::stream_destroy(s_); s_ = nullptr; }
    int create() { release(); return ZKV_DEVMEM_API::stream_create(&s_) ? ZKV_OK : ZKV_ERR_HIP; }
    operator ZKV_DEVMEM_API::stream_t() const { return s_; }
};

}  // namespace zkv
