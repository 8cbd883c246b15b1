// mp_hip_own.h — scoped owners of what the host side gets from the HIP runtime: device blocks, pinned blocks, events and the
// library's own stream.  Host only.  These are the ONLY callers of the HIP release functions in csrc/ (tests/test_hip_ownership.py):
// a handle holds holders or documented views, a one-shot entry point holds locals, and every early return is clean.
// Move-only and nothing more: no pool, no sizes, no counting.  Releasing a device block synchronises the device, so holders are
// (re)allocated and destroyed where the code did that before — creation, re-sizing, destruction — never per step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include <utility>

template <class T, class Release>
class mp_owned {
    T* p_ = nullptr;

public:
    mp_owned() = default;
    mp_owned(mp_owned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    mp_owned& operator=(mp_owned&& o) noexcept { swap(o); o.reset(); return *this; }
    mp_owned(const mp_owned&) = delete;
    mp_owned& operator=(const mp_owned&) = delete;
    ~mp_owned() { reset(); }
    void reset() { if (p_) Release()(p_); p_ = nullptr; }
    void swap(mp_owned& o) noexcept { std::swap(p_, o.p_); }
    T* get() const { return p_; }
    operator T*() const { return p_; }   // launch sites and PropagateArgs assignments read as with a raw pointer
    T* operator->() const { return p_; }
    T** put() { reset(); return &p_; }   // for the allocating call: releases what was held, null if that call fails
};
template <class T, class R>
void swap(mp_owned<T, R>& a, mp_owned<T, R>& b) noexcept { a.swap(b); }

struct mp_release_dev { void operator()(void* p) const { (void)hipFree(p); } };
struct mp_release_pinned { void operator()(void* p) const { (void)hipHostFree(p); } };
struct mp_release_event { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

template <class T> using mp_dev = mp_owned<T, mp_release_dev>;        // a hipMalloc block of T
template <class T> using mp_pinned = mp_owned<T, mp_release_pinned>;  // a hipHostMalloc block of T
using mp_event = mp_owned<std::remove_pointer_t<hipEvent_t>, mp_release_event>;

// `count` elements of T (bytes when T is a byte type).  Under HIPCK and its kin the message of a failure still names hipMalloc.
template <class T>
hipError_t mp_hipMalloc(mp_dev<T>& d, size_t count) { return hipMalloc(reinterpret_cast<void**>(d.put()), sizeof(T) * count); }
template <class T>
hipError_t mp_hipHostMalloc(mp_pinned<T>& d, size_t count, unsigned flags = hipHostMallocDefault) {
    return hipHostMalloc(reinterpret_cast<void**>(d.put()), sizeof(T) * count, flags);
}
inline hipError_t mp_hipEventCreate(mp_event& e, unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(e.put(), flags); }

// The stream a handle works on: the caller's (borrowed) or one of the library's own (destroyed with the holder).
class mp_hip_stream {
    hipStream_t s_ = nullptr;
    bool own_ = false;

public:
    mp_hip_stream() = default;
    mp_hip_stream(const mp_hip_stream&) = delete;
    mp_hip_stream& operator=(const mp_hip_stream&) = delete;
    ~mp_hip_stream() { if (own_) (void)hipStreamDestroy(s_); }
    void borrow(hipStream_t s) { s_ = s; }   // (once, on a fresh holder)
    hipError_t create(unsigned flags) {
        const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
        own_ = e == hipSuccess;
        return e;
    }
    operator hipStream_t() const { return s_; }
};
