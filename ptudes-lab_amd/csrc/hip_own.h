// hip_own.h -- who frees what the host library (ptudes_mi.hip) takes from the HIP runtime.  Host code only.
// Members are destroyed in reverse order of declaration: a handle declares its streams first, its events next and its memory last.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include <vector>

// Device memory and pinned host words.  Every handle has one: it fills the raw pointer fields the handle and the kernel context already
// have, remembers each pointer with its byte count and frees them all when the handle is deleted.  A local one is a scoped temporary:
// whichever way the function returns, its buffers go back.  In counting mode the requests are only added up, so that the footprint of a
// handle is what its allocation function asks for and not a second formula.
class DevOwner {
    struct Held { void* p; size_t bytes; bool pinned; };
    std::vector<Held> held_;
    size_t bytes_ = 0;
    bool counting_;
    hipError_t take(void** p, size_t bytes, bool pinned) {
        *p = nullptr;
        bytes_ += bytes;
        if (counting_) return hipSuccess;
        const hipError_t e = pinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes);
        if (e != hipSuccess) {  // (the runtime's sticky "last error" is cleared: a later check would report it as its own)
            (void)hipGetLastError();
            *p = nullptr;
            if (err == hipSuccess) err = e;
            return e;
        }
        held_.push_back({*p, bytes, pinned});
        return hipSuccess;
    }
    static void give_back(const Held& h) { if (h.pinned) (void)hipHostFree(h.p); else (void)hipFree(h.p); }
    size_t find(const void* p) const {
        size_t i = 0;
        while (i < held_.size() && held_[i].p != p) ++i;
        return i;
    }

public:
    hipError_t err = hipSuccess;  // the first request that failed, for the functions that make a list of them and look once
    explicit DevOwner(bool counting = false) : counting_(counting) {}
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    ~DevOwner() { for (const Held& h : held_) give_back(h); }

    // n elements for *p: alloc for a request that is checked on its own; add for one of a list that is judged once, by `err` (what
    // follows a failed request of the list is not asked for any more)
    template <typename T> hipError_t alloc(T** p, size_t n) { return take((void**)p, n * sizeof(T), false); }
    template <typename T> void add(T** p, size_t n) { *p = nullptr; if (err == hipSuccess) (void)take((void**)p, n * sizeof(T), false); }
    template <typename T> void add_pinned(T** p, size_t n) { *p = nullptr; if (err == hipSuccess) (void)take((void**)p, n * sizeof(T), true); }
    size_t requested() const { return bytes_; }  // bytes asked for so far (counting mode: nothing else happens)
    size_t bytes_of(const void* p) const { const size_t i = find(p); return i < held_.size() ? held_[i].bytes : 0; }
    // frees one buffer (null or unknown: nothing) and clears the field
    template <typename T> void release(T** p) {
        const size_t i = find(*p);
        if (*p && i < held_.size()) { give_back(held_[i]); held_.erase(held_.begin() + (long)i); }
        *p = nullptr;
    }
    // a buffer that grew: `np`, allocated by `from` (a scoped temporary until here), takes the place of *p
    template <typename T> void replace(T** p, DevOwner& from, T* np) {
        release(p);
        const size_t i = from.find(np);
        if (i < from.held_.size()) { held_.push_back(from.held_[i]); from.held_.erase(from.held_.begin() + (long)i); }
        *p = np;
    }
};

// A stream or an event: move-only, destroyed with its handle, used wherever the raw hipStream_t / hipEvent_t is
template <typename H, hipError_t (*Destroy)(H)>
class HipHandle {
protected:
    H h_ = nullptr;
    bool own_ = true;
public:
    HipHandle() = default;
    HipHandle(HipHandle&& o) noexcept : h_(o.h_), own_(o.own_) { o.h_ = nullptr; }
    ~HipHandle() { reset(); }
    void reset() { if (h_ && own_) (void)Destroy(h_); h_ = nullptr; }
    operator H() const { return h_; }
};
struct Stream : HipHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { reset(); own_ = true; return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
    void borrow(hipStream_t s) { reset(); own_ = false; h_ = s; }  // a runner's stream: used, never destroyed
};
struct Event : HipHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDisableTiming) { reset(); return hipEventCreateWithFlags(&h_, flags); }
};

// Times the dominant kernel: begin / end around a launch record a pair of events (more are made as needed), collect() - after the
// stream has been waited for - adds up the pairs recorded since the last one.
struct GnTimer {
    bool on = false;
    double ms = 0;
    int64_t launches = 0;
    hipError_t begin(hipStream_t s, bool this_launch = true) {
        armed_ = on && this_launch;
        if (!armed_) return hipSuccess;
        while (used_ + 2 > ev_.size()) {
            Event e;
            const hipError_t rc = e.create(hipEventDefault);
            if (rc != hipSuccess) { armed_ = false; return rc; }
            ev_.push_back(std::move(e));
        }
        return hipEventRecord(ev_[used_], s);
    }
    hipError_t end(hipStream_t s) {
        if (!armed_) return hipSuccess;
        armed_ = false;
        used_ += 2;
        return hipEventRecord(ev_[used_ - 1], s);
    }
    void collect() {
        for (size_t i = 0; i + 1 < used_; i += 2) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev_[i], ev_[i + 1]) == hipSuccess) { ms += t; launches++; }
        }
        used_ = 0;
    }
    // ptl_*_profile: the totals so far, then reset and switch as asked (the caller has waited for the stream)
    void report(int enable, double* ms_total, int64_t* n_launches, int reset) {
        collect();
        if (ms_total) *ms_total = ms;
        if (n_launches) *n_launches = launches;
        if (reset) { ms = 0; launches = 0; }
        on = enable != 0;
    }

private:
    std::vector<Event> ev_;
    size_t used_ = 0;
    bool armed_ = false;
};
