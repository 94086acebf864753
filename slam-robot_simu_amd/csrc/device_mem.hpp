// device_mem.hpp -- the one owner of device memory, pinned host memory and
// events ("Resource ownership").  Every handle holds a DeviceMem;
// whatever it allocated goes when the handle is deleted, so a create that
// fails half way leaks nothing.  No other file calls the allocation entry
// points of the runtime.
#pragma once

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.hpp"

namespace slam {

// Live resources of this library in this process (slam_debug_live_resources).
struct LiveResources {
    std::atomic<int64_t> device_bytes{0}, pinned_bytes{0}, events{0};
};
inline LiveResources g_live;

class DeviceMem {
public:
    DeviceMem() = default;
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    DeviceMem(DeviceMem&& o) noexcept { swap(o); }
    DeviceMem& operator=(DeviceMem&& o) noexcept {
        if (this != &o) {
            clear();
            swap(o);
        }
        return *this;
    }
    ~DeviceMem() { clear(); }

    // count elements of device memory (a zero-byte request allocates 8 bytes);
    // *p is the base pointer the owner records -- the caller may offset its copy
    // flags: hipExtMallocWithFlags' (fine-grained memory), 0 for plain memory
    template <typename T>
    int alloc(T** p, size_t count, unsigned flags = 0) {
        const size_t bytes = count * sizeof(T) ? count * sizeof(T) : 8;
        void* q = nullptr;
        if (flags)
            SLAM_HIP_TRY(hipExtMallocWithFlags(&q, bytes, flags));
        else
            SLAM_HIP_TRY(hipMalloc(&q, bytes));
        blocks_.push_back({q, bytes, false});
        g_live.device_bytes += (int64_t)bytes;
        *p = static_cast<T*>(q);
        return SLAM_OK;
    }

    // count elements of pinned host memory; with dev (nullable), its device
    // address too
    template <typename T>
    int alloc_pinned(T** host, std::add_pointer_t<T*> dev, size_t count, unsigned flags) {
        const size_t bytes = count * sizeof(T);
        void* q = nullptr;
        SLAM_HIP_TRY(hipHostMalloc(&q, bytes, flags));
        blocks_.push_back({q, bytes, true});
        g_live.pinned_bytes += (int64_t)bytes;
        *host = static_cast<T*>(q);
        if (dev) SLAM_HIP_TRY(hipHostGetDevicePointer((void**)dev, q, 0));
        return SLAM_OK;
    }

    // free one recorded base pointer now (device or pinned) and null it
    template <typename T>
    void release(T*& p) {
        if (!p) return;
        const auto it = std::find_if(blocks_.begin(), blocks_.end(),
                                     [&](const Block& b) { return b.p == (void*)p; });
        if (it != blocks_.end()) {
            free_block(*it);
            blocks_.erase(it);
        }
        p = nullptr;
    }

    int event(hipEvent_t* e) {
        SLAM_HIP_TRY(hipEventCreate(e));
        events_.push_back(*e);
        ++g_live.events;
        return SLAM_OK;
    }

    void clear() {
        for (const Block& b : blocks_) free_block(b);
        blocks_.clear();
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
        g_live.events -= (int64_t)events_.size();
        events_.clear();
    }

private:
    struct Block {
        void* p;
        size_t bytes;
        bool pinned;
    };
    static void free_block(const Block& b) {
        if (b.pinned) {
            (void)hipHostFree(b.p);
            g_live.pinned_bytes -= (int64_t)b.bytes;
        } else {
            (void)hipFree(b.p);
            g_live.device_bytes -= (int64_t)b.bytes;
        }
    }
    void swap(DeviceMem& o) noexcept {
        blocks_.swap(o.blocks_);
        events_.swap(o.events_);
    }
    std::vector<Block> blocks_;
    std::vector<hipEvent_t> events_;
};

// What a create holds its new handle in until it has succeeded: every early
// return then goes through the handle's own destroy.
template <typename H, int (*Destroy)(H*)>
struct HandleDeleter {
    void operator()(H* h) const { (void)Destroy(h); }
};
template <typename H, int (*Destroy)(H*)>
using HandlePtr = std::unique_ptr<H, HandleDeleter<H, Destroy>>;

// Process-lifetime scratch of the stateless entry points: per device one
// stream and one growing buffer, used under its mutex.  Never destroyed (the
// runtime may be gone at static destruction); growth goes through DeviceMem,
// so it is counted.
struct StaticScratch {
    std::mutex mu;
    size_t cap = 0;      // in the caller's units
    char* buf = nullptr;
    hipStream_t stream = nullptr;
    DeviceMem mem;

    // with mu held: select the device, make the stream, hold >= units
    int begin(int device, size_t units, size_t unit_bytes) {
        SLAM_HIP_TRY(hipSetDevice(device));
        if (!stream) SLAM_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (units <= cap) return SLAM_OK;
        mem.release(buf);
        cap = 0;
        const int rc = mem.alloc(&buf, units * unit_bytes);
        if (rc) return rc;
        cap = units;
        return SLAM_OK;
    }
};

// one set per entry-point family (Tag), indexed by device
template <typename Tag>
StaticScratch& static_scratch(int device) {
    static StaticScratch* const s = new StaticScratch[64];
    return s[device & 63];
}

}  // namespace slam
