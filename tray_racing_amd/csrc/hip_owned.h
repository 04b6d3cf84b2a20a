// hip_owned.h - move-only owners of the HIP resources the C ABI holds (device and pinned host memory, events, streams;
// the refit's stream-ordered staging buffer).  A destructor releases its resource and ignores the error, as a teardown
// must; kernel parameter structs take the raw pointer with get().  Not installed; not part of the ABI.
#ifndef TRX_HIP_OWNED_H
#define TRX_HIP_OWNED_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace trxapi {

// The shared move-only shell: R holds the resource type, the null value and the release call.
template <typename R>
class Owned {
  public:
    using T = typename R::Type;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = T(), o.n_ = 0; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_, n_ = o.n_;
            o.h_ = T(), o.n_ = 0;
        }
        return *this;
    }
    ~Owned() { reset(); }
    T get() const { return h_; }
    uint64_t count() const { return n_; } // elements of a buffer
    explicit operator bool() const { return h_ != T(); }
    void reset() {
        if (h_ != T()) R::release(h_);
        h_ = T(), n_ = 0;
    }
    // gives the resource up without releasing it (a table a kernel may still read is kept rather than freed)
    T release() {
        const T h = h_;
        h_ = T(), n_ = 0;
        return h;
    }

  protected:
    hipError_t take(hipError_t e, T h, uint64_t n) { // a failed creation leaves the owner empty with count 0
        if (e == hipSuccess) h_ = h, n_ = n;
        return e;
    }
    T h_ = T();
    uint64_t n_ = 0;
};

template <typename E>
struct DevRelease {
    using Type = E *;
    static void release(E *p) { (void)hipFree(p); }
};
// hipMalloc memory of `count()` elements of E
template <typename E>
struct DevBuf : Owned<DevRelease<E>> {
    hipError_t alloc(uint64_t n) {
        this->reset();
        E *p = nullptr;
        return this->take(hipMalloc((void **)&p, n * sizeof(E)), p, n);
    }
    // a request beyond the current count frees the buffer, then allocates exactly n elements (no headroom)
    hipError_t grow(uint64_t n) { return n > this->count() ? alloc(n) : hipSuccess; }
};

template <typename E>
struct HostRelease {
    using Type = E *;
    static void release(E *p) { (void)hipHostFree(p); }
};
// hipHostMalloc memory of `count()` elements of E
template <typename E>
struct HostBuf : Owned<HostRelease<E>> {
    hipError_t alloc(uint64_t n, unsigned flags) {
        this->reset();
        E *p = nullptr;
        return this->take(hipHostMalloc((void **)&p, n * sizeof(E), flags), p, n);
    }
};

// hipMallocAsync memory, freed in the order of the stream it was allocated on (a temporary of that stream's work)
template <typename E>
class StreamBuf {
  public:
    StreamBuf() = default;
    StreamBuf(const StreamBuf &) = delete;
    StreamBuf &operator=(const StreamBuf &) = delete;
    ~StreamBuf() { (void)reset(); }
    E *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    hipError_t alloc(uint64_t n, hipStream_t stream) {
        (void)reset();
        E *p = nullptr;
        const hipError_t e = hipMallocAsync((void **)&p, n * sizeof(E), stream);
        if (e == hipSuccess) p_ = p, stream_ = stream;
        return e;
    }
    hipError_t reset() {
        const hipError_t e = p_ ? hipFreeAsync(p_, stream_) : hipSuccess;
        p_ = nullptr;
        return e;
    }

  private:
    E *p_ = nullptr;
    hipStream_t stream_ = nullptr;
};

struct EventRelease {
    using Type = hipEvent_t;
    static void release(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct Event : Owned<EventRelease> {
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        hipEvent_t e = nullptr;
        return take(hipEventCreateWithFlags(&e, flags), e, 0);
    }
};

struct StreamRelease {
    using Type = hipStream_t;
    static void release(hipStream_t s) { (void)hipStreamDestroy(s); }
};
struct Stream : Owned<StreamRelease> {
    hipError_t create(unsigned flags) {
        reset();
        hipStream_t s = nullptr;
        return take(hipStreamCreateWithFlags(&s, flags), s, 0);
    }
};

} // namespace trxapi

#endif // TRX_HIP_OWNED_H
